/*
 * ksw2_host_sga.c -- semi-global alignment with the interval's start and a CIGAR: ksw2amd_sg_align_batch / ksw2amd_sg_align_batch_flat /
 * ksw2amd_sg_align (include/ksw2_amd.h).  What a caller of ksw2amd_sg_batch does by hand -- reverse the query and
 * target[0..te] on the host, an extension call for where the whole reversed query ends, another for the CIGAR -- as one call in three stages:
 *   1. the forward pass of ksw2amd_sg_batch: score, qe = qlen - 1, te;
 *   2. the anchored start pass, launched behind it on what it left in device memory -- task table, pen tables, sequences, results; no
 *      download, host reversal or second upload in between (k2a_shim_launch_sg_rev, handed to ll_batch_ex as its ll_rev_fn): the largest tb
 *      at which the whole query against target[tb..te] scores `score` globally, te + 1 for the empty interval;
 *   3. the CIGAR of the pairs with a non-empty interval: the scalar-contract ksw_extz, unbanded, on query x target[tb..te] through the batch
 *      machinery of ksw2amd_extz_batch.  Its score must equal the semi-global score: anything else is reported as an internal error.  An
 *      empty interval's CIGAR, qlen I, is written here.
 *
 * This is the only host object that refers to k2a_shim_launch_sg_rev (it names k2a_shim_launch_sg too, like ksw2_host_sg.c).
 * The two-piece entries (ksw2_host_sgd.c) run the same three stages through sga_align_ex / sga_align_flat_ex with
 * their own two launches and an ll_dual_t: stage 3 is then the scalar-contract ksw_extd.
 * The overlap entries (ksw2_host_ova.c) run them with ft->ov: the start pass may then name a start (0, qb) in row 0,
 * which ova_cells admits, and stage 3 aligns query[qb..qe]; an empty query interval's CIGAR, (te + 1) D, is written here.  With qb = 0
 * everything below is what it was.
 */
#include "ksw2_host_int.h"

void sga_reset(int n, ksw2amd_laln_t *aln)
{
	int i;
	for (i = 0; aln && i < n; ++i) { aln[i].score = 0; aln[i].qb = aln[i].qe = aln[i].tb = aln[i].te = -1; aln[i].n_cigar = 0; }
}

/* both intervals non-empty (qb > qe: the overlap entries' empty query interval; qb = 0 in the semi-global ones) */
static inline int sga_has_interval(const ksw2amd_laln_t *a) { return a->qe >= 0 && a->te >= 0 && a->tb <= a->te && a->qb <= a->qe; }

/* after stages 1 and 2: aln[i] = score, the query's ends and the interval, the start pass checked against the forward pass (no CIGAR
 * yet).  qlen / tlen: the pairs' lengths, `stride` ints apart.  Returns through *na the pairs with a non-empty interval */
int sga_cells(int n, const int32_t *qlen, const int32_t *tlen, size_t stride, const ksw2amd_lres_t *res, const K2aLLBeg *beg, ksw2amd_laln_t *aln, int *na_)
{
	int i, na = 0;
	char msg[96];
	for (i = 0; i < n; ++i) {
		ksw2amd_laln_t *a = &aln[i];
		const int ql = qlen[i * stride], tl = tlen[i * stride];
		a->score = res[i].score; a->qe = res[i].qe; a->te = res[i].te; a->qb = beg[i].qb; a->tb = beg[i].tb;
		a->n_cigar = 0;
		if (ql <= 0) { a->score = 0; a->qb = a->qe = a->tb = a->te = -1; continue; }
		if (tl <= 0) { a->qb = 0; a->tb = 0; continue; }               /* the whole query inserted before the target: te = -1, empty interval */
		/* the best global score of the query against an interval that ends in te is the forward score itself */
		if (beg[i].score != res[i].score || beg[i].qb != 0 || beg[i].tb < 0 || beg[i].tb > res[i].te + 1) {
			snprintf(msg, sizeof(msg), "%d: forward %d, reversed %d (tb %d, te %d)", i, res[i].score, beg[i].score, beg[i].tb, res[i].te);
			return fail(KSW2AMD_E_NODEVICE, "semi-global alignment: internal error, start pass disagrees with the forward pass on pair %s", msg);
		}
		na += sga_has_interval(a);
	}
	*na_ = na;
	return KSW2AMD_OK;
}

/* the same for the overlap entries (ksw2amd_ov_align_batch): the start pass may name exactly the candidate cells --
 * (tb, 0) with 0 <= tb <= te + 1, or, with the query's start free, (0, qb) with 0 <= qb <= qe + 1 -- with the forward pass's score */
static int ova_cells(int n, const int32_t *qlen, const int32_t *tlen, size_t stride, int ends, const ksw2amd_lres_t *res, const K2aLLBeg *beg, ksw2amd_laln_t *aln, int *na_)
{
	int i, na = 0;
	char msg[128];
	for (i = 0; i < n; ++i) {
		ksw2amd_laln_t *a = &aln[i];
		const int ql = qlen[i * stride], tl = tlen[i * stride];
		a->score = res[i].score; a->qe = res[i].qe; a->te = res[i].te; a->qb = beg[i].qb; a->tb = beg[i].tb;
		a->n_cigar = 0;
		if (ql <= 0) { a->score = 0; a->qb = a->qe = a->tb = a->te = -1; continue; }
		if (tl <= 0) { a->qb = (ends & KSW2AMD_OV_QBEG) ? ql : 0; a->tb = 0; continue; }      /* te = -1: the query inserted, or all of it hanging over */
		if (beg[i].score != res[i].score
		    || !((beg[i].qb == 0 && beg[i].tb >= 0 && beg[i].tb <= res[i].te + 1)
		         || ((ends & KSW2AMD_OV_QBEG) && beg[i].tb == 0 && beg[i].qb >= 0 && beg[i].qb <= res[i].qe + 1))) {
			snprintf(msg, sizeof(msg), "%d: forward %d, reversed %d (qb %d, tb %d, qe %d, te %d)", i, res[i].score, beg[i].score, beg[i].qb, beg[i].tb, res[i].qe, res[i].te);
			return fail(KSW2AMD_E_NODEVICE, "overlap alignment: internal error, start pass disagrees with the forward pass on pair %s", msg);
		}
		na += sga_has_interval(a);
	}
	*na_ = na;
	return KSW2AMD_OK;
}

/* stage 3.  Empty intervals: (qe + 1) I for an empty target interval, (te + 1) D for an empty query interval (overlap entries), written here.  The na pairs with an interval: query x target[tb..te] as extension pairs into HOST
 * memory; the caller's CIGAR buffers travel through ez[] and back.  at_start = 0: pairs[i].query / target are the full sequences; 1: they already point
 * at residues qb / tb (the intervals of a device arena, brought back).  qb = 0 in the semi-global entries.  du: the scalar ksw_extd
 * with (gapo2, gape2), the pieces in the caller's order, instead of ksw_extz */
int sga_cigars(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lpair_t *pairs, int at_start, int na, ksw2amd_laln_t *aln,
               const ll_dual_t *du)
{
	ksw2amd_pair_t *pp = 0;
	ksw_extz_t *ez = 0;
	int32_t *idx = 0;
	int i, k, rc = KSW2AMD_OK;
	char msg[96];
	for (i = 0; i < n; ++i) {
		ksw2amd_laln_t *a = &aln[i];
		ksw_extz_t z;
		if (a->qe < 0 || sga_has_interval(a) || (a->qb > a->qe && a->te < 0)) continue;      /* (the last: all of the query hangs over no target) */
		z.cigar = a->cigar; z.m_cigar = a->m_cigar;
		ez_reserve(km, &z, 1);
		a->cigar = z.cigar; a->m_cigar = z.m_cigar;
		if (!a->cigar) { a->m_cigar = 0; return fail(KSW2AMD_E_NOMEM, "semi-global alignment: host allocation failed%s", ""); }
		a->cigar[0] = a->qb > a->qe ? (uint32_t)(a->te + 1) << 4 | 2u : (uint32_t)(a->qe + 1) << 4 | 1u;
		a->n_cigar = 1;
	}
	if (na == 0) return KSW2AMD_OK;
	pp = (ksw2amd_pair_t*)malloc(sizeof(*pp) * (size_t)na);
	ez = (ksw_extz_t*)calloc((size_t)na, sizeof(*ez));
	idx = (int32_t*)malloc(sizeof(*idx) * (size_t)na);
	if (!pp || !ez || !idx) { rc = fail(KSW2AMD_E_NOMEM, "semi-global alignment: host allocation failed%s", ""); goto out; }
	for (i = 0, k = 0; i < n; ++i) {
		const ksw2amd_laln_t *a = &aln[i];
		if (!sga_has_interval(a)) continue;
		pp[k].query = pairs[i].query + (at_start ? 0 : a->qb); pp[k].qlen = a->qe - a->qb + 1;
		pp[k].target = pairs[i].target + (at_start ? 0 : a->tb); pp[k].tlen = a->te - a->tb + 1;
		pp[k].w = -1; pp[k].zdrop = -1; pp[k].end_bonus = 0;
		pp[k].flag = KSW_EZ_GENERIC_SC | (flag & (KSW_EZ_RIGHT | KSW_EZ_REV_CIGAR));
		ez[k].cigar = a->cigar; ez[k].m_cigar = a->m_cigar;
		idx[k++] = i;
	}
	{
		ksw2amd_scoring_t sc;
		sc.m = m; sc.mat = mat; sc.q = (int8_t)gapo; sc.e = (int8_t)gape; sc.q2 = (int8_t)(du ? du->gapo2 : 0); sc.e2 = (int8_t)(du ? du->gape2 : 0);
		rc = ext_batch_scalar(du != 0, km, &sc, na, pp, ez);
	}
	for (k = 0; k < na; ++k) {                 /* the buffers may have grown or moved: always hand them back */
		ksw2amd_laln_t *a = &aln[idx[k]];
		a->cigar = ez[k].cigar; a->m_cigar = ez[k].m_cigar;
		a->n_cigar = rc == KSW2AMD_OK ? ez[k].n_cigar : 0;
	}
	for (k = 0; k < na && rc == KSW2AMD_OK; ++k)
		if (ez[k].score != aln[idx[k]].score) {
			snprintf(msg, sizeof(msg), "%d: semi-global %d, global %d", (int)idx[k], aln[idx[k]].score, ez[k].score);
			rc = fail(KSW2AMD_E_NODEVICE, "semi-global alignment: internal error, the interval's global score differs from the semi-global score on pair %s", msg);
		}
out:
	free(pp); free(ez); free(idx);
	return rc;
}

int sga_check_flag(int flag)
{
	if (flag & ~LLA_FLAGS) return fail(KSW2AMD_E_PARAM, "semi-global alignment: flag accepts KSW_EZ_SCORE_ONLY, KSW_EZ_RIGHT and KSW_EZ_REV_CIGAR only%s", "");
	return KSW2AMD_OK;
}

/* ksw2amd_sg_align_batch with the two launches (ft->launch, rev) and the two-piece cost (du, or NULL) as parameters */
int sga_align_ex(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln,
                 const ll_fit_t *ft, ll_rev_fn rev, const ll_dual_t *du)
{
	ksw2amd_lres_t *res = 0;
	K2aLLBeg *beg = 0;
	int na = 0, rc;
	/* every argument before anything is staged: the flag here, m / mat / gap costs / pair array / ranges / residue codes in ll_batch_ex */
	if ((rc = sga_check_flag(flag)) != KSW2AMD_OK) return rc;
	if (n > 0 && !aln) return fail(KSW2AMD_E_PARAM, "semi-global alignment: bad pair array%s", "");
	if (n > 0) {
		res = (ksw2amd_lres_t*)malloc(sizeof(*res) * (size_t)n);
		beg = (K2aLLBeg*)malloc(sizeof(*beg) * (size_t)n);
		if (!res || !beg) { rc = fail(KSW2AMD_E_NOMEM, "semi-global alignment: host allocation failed%s", ""); goto out; }
	}
	if ((rc = ll_batch_ex(m, mat, gapo, gape, n, pairs, res, rev, beg, 0, 0, du, ft)) != KSW2AMD_OK) goto out;
	if (n == 0) goto out;
	if ((rc = ft->ov ? ova_cells(n, &pairs[0].qlen, &pairs[0].tlen, sizeof(pairs[0]) / sizeof(int32_t), ft->ends, res, beg, aln, &na)
	                 : sga_cells(n, &pairs[0].qlen, &pairs[0].tlen, sizeof(pairs[0]) / sizeof(int32_t), res, beg, aln, &na)) != KSW2AMD_OK) goto out;
	if (flag & KSW_EZ_SCORE_ONLY) goto out;
	rc = sga_cigars(km, m, mat, gapo, gape, flag, n, pairs, 0, na, aln, du);
out:
	if (rc != KSW2AMD_OK) sga_reset(n, aln);
	free(res); free(beg);
	return rc;
}

int ksw2amd_sg_align_batch(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln)
{
	ll_fit_t ft;
	ft.launch = k2a_shim_launch_sg; ft.ov = ft.ends = 0;
	return sga_align_ex(km, m, mat, gapo, gape, flag, n, pairs, aln, &ft, k2a_shim_launch_sg_rev, 0);
}

/* ksw2amd_sg_align_batch_flat, parameterised the same way */
int sga_align_flat_ex(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lflat_t *in, ksw2amd_laln_t *aln,
                      const ll_fit_t *ft, ll_rev_fn rev, const ll_dual_t *du)
{
	ksw2amd_lres_t *res = 0;
	K2aLLBeg *beg = 0;
	ksw2amd_lpair_t *pp = 0;
	uint8_t *host = 0;
	int i, na = 0, rc;
	if ((rc = sga_check_flag(flag)) != KSW2AMD_OK) return rc;
	if (n > 0 && !aln) return fail(KSW2AMD_E_PARAM, "semi-global alignment: bad flat batch arguments%s", "");
	if (n > 0) {
		res = (ksw2amd_lres_t*)malloc(sizeof(*res) * (size_t)n);
		beg = (K2aLLBeg*)malloc(sizeof(*beg) * (size_t)n);
		if (!res || !beg) { rc = fail(KSW2AMD_E_NOMEM, "semi-global alignment: host allocation failed%s", ""); goto out; }
	}
	/* stages 1 and 2 on the borrowed arena */
	if ((rc = llf_batch_ex(m, mat, gapo, gape, n, in, res, rev, beg, 0, 0, du, ft)) != KSW2AMD_OK) goto out;
	if (n == 0) goto out;
	if ((rc = ft->ov ? ova_cells(n, in->qlen, in->tlen, 1, ft->ends, res, beg, aln, &na) : sga_cells(n, in->qlen, in->tlen, 1, res, beg, aln, &na)) != KSW2AMD_OK) goto out;
	if (flag & KSW_EZ_SCORE_ONLY) goto out;
	/* stage 3: [qoff + qb, qoff + qe] (semi-global: the whole query) x [toff + tb, toff + te] under the scalar ksw_extz (du: ksw_extd) contract.  Host arena: pointers into it.  Device arena: the
	 * span of the aligned intervals and their queries comes back in one copy, then the same pointer path */
	pp = (ksw2amd_lpair_t*)malloc(sizeof(*pp) * (size_t)n);
	if (!pp) { rc = fail(KSW2AMD_E_NOMEM, "semi-global alignment: host allocation failed%s", ""); goto out; }
	if (in->on_device && na > 0) {
		uint64_t lo = UINT64_MAX, hi = 0;
		void *st = thread_stream();
		for (i = 0; i < n; ++i) {
			const ksw2amd_laln_t *a = &aln[i];
			if (!sga_has_interval(a)) continue;
			if (in->qoff[i] + (uint64_t)a->qb < lo) lo = in->qoff[i] + (uint64_t)a->qb;
			if (in->toff[i] + (uint64_t)a->tb < lo) lo = in->toff[i] + (uint64_t)a->tb;
			if (in->qoff[i] + (uint64_t)a->qe + 1 > hi) hi = in->qoff[i] + (uint64_t)a->qe + 1;
			if (in->toff[i] + (uint64_t)a->te + 1 > hi) hi = in->toff[i] + (uint64_t)a->te + 1;
		}
		host = (uint8_t*)malloc((size_t)(hi - lo));
		if (!host) { rc = fail(KSW2AMD_E_NOMEM, "semi-global alignment: host allocation failed%s", ""); goto out; }
		if (!st || k2a_shim_d2h(host, in->base + lo, (size_t)(hi - lo), st) || k2a_shim_stream_sync(st)) { rc = fail(KSW2AMD_E_NODEVICE, "semi-global alignment: %s", k2a_shim_last_error()); goto out; }
		for (i = 0; i < n; ++i) {
			const ksw2amd_laln_t *a = &aln[i];
			pp[i].query = pp[i].target = 0; pp[i].qlen = in->qlen[i]; pp[i].tlen = in->tlen[i];
			if (!sga_has_interval(a)) continue;
			pp[i].query = host + (in->qoff[i] + (uint64_t)a->qb - lo); pp[i].target = host + (in->toff[i] + (uint64_t)a->tb - lo);
		}
	} else
		for (i = 0; i < n; ++i) {                 /* (a device arena without an interval: the pointers are never followed) */
			pp[i].query = in->base + in->qoff[i]; pp[i].target = in->base + in->toff[i]; pp[i].qlen = in->qlen[i]; pp[i].tlen = in->tlen[i];
		}
	rc = sga_cigars(km, m, mat, gapo, gape, flag, n, pp, in->on_device != 0, na, aln, du);
out:
	if (rc != KSW2AMD_OK) sga_reset(n, aln);
	free(res); free(beg); free(pp); free(host);
	return rc;
}

int ksw2amd_sg_align_batch_flat(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lflat_t *in, ksw2amd_laln_t *aln)
{
	ll_fit_t ft;
	ft.launch = k2a_shim_launch_sg; ft.ov = ft.ends = 0;
	return sga_align_flat_ex(km, m, mat, gapo, gape, flag, n, in, aln, &ft, k2a_shim_launch_sg_rev, 0);
}

/* one pair on a ksw_ll_qinit profile: entry 0 of ksw2amd_sg_align_batch, failures reported like ksw_ll_i16 */
int ksw2amd_sg_align(void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int flag, ksw2amd_laln_t *aln)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	int rc;
	sga_reset(aln ? 1 : 0, aln);
	if (!p || !aln) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_sg_align: NULL profile or result%s", ""); call_failed("ksw2amd_sg_align", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_sg_align_batch(km, p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, flag, 1, &pr, aln);
	if (rc != KSW2AMD_OK) { call_failed("ksw2amd_sg_align", rc, 0); return 0; }
	return aln->score;
}
