/*
 * ksw2_host_lla.c -- local alignment with start cell and CIGAR: ksw2amd_ll_align_batch / ksw2amd_ll_align (include/ksw2_amd.h, DESIGN.md
 * section 3.15).  What a minimap2 / BWA style caller does by hand around ksw_ll_i16 -- forward pass, reverse both prefixes, second pass,
 * global alignment of the interval -- as one call in three stages:
 *   1. the forward pass of ksw2amd_ll_batch (ksw2_host_ll.c): score, qe, te;
 *   2. the start-cell pass, launched behind it on what it left in device memory -- task table, pen tables, sequences, results; no
 *      download, host reversal or second upload in between (k2a_shim_launch_ll_rev, handed to ll_batch_ex as a function pointer);
 *   3. the CIGAR: the scalar-contract ksw_extz, unbanded, on query[qb..qe] x target[tb..te] through the batch machinery of
 *      ksw2amd_extz_batch.  Its global score must equal the local score: anything else is reported as an internal error.
 *
 * This is the only host object that refers to k2a_shim_launch_ll_rev.
 */
#include "ksw2_host_int.h"

/* after stages 1 and 2: aln[i] = score and both cells, checked against each other (no CIGAR yet).  Returns through *na the pairs with a
 * positive score */
int lla_cells(int n, const ksw2amd_lres_t *res, const K2aLLBeg *beg, ksw2amd_laln_t *aln, int *na_)
{
	int i, na = 0;
	char msg[96];
	for (i = 0; i < n; ++i) {
		ksw2amd_laln_t *a = &aln[i];
		a->score = res[i].score; a->qe = res[i].qe; a->te = res[i].te; a->qb = beg[i].qb; a->tb = beg[i].tb;
		a->n_cigar = 0;
		if (res[i].score <= 0) { a->score = 0; a->qb = a->qe = a->tb = a->te = -1; continue; }
		/* (qe, te) is the only cell of its prefix rectangle that holds the score, so the reversed pass finds the same one */
		if (beg[i].score != res[i].score || beg[i].qb < 0 || beg[i].qb > res[i].qe || beg[i].tb < 0 || beg[i].tb > res[i].te) {
			snprintf(msg, sizeof(msg), "%d: forward %d, reversed %d", i, res[i].score, beg[i].score);
			return fail(KSW2AMD_E_NODEVICE, "local alignment: internal error, start-cell pass disagrees with the forward pass on pair %s", msg);
		}
		++na;
	}
	*na_ = na;
	return KSW2AMD_OK;
}

/* stage 3 for the na pairs of aln[] with a positive score: the sub-ranges as extension pairs into HOST memory; the caller's CIGAR
 * buffers travel through ez[] and back.  at_start = 0: pairs[i] are the full sequences; 1: pairs[i].query / .target already point at
 * residues qb / tb (ksw2_host_llf.c: the intervals of a device arena, brought back) */
int lla_cigars(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lpair_t *pairs, int at_start, int na, ksw2amd_laln_t *aln,
               const ll_dual_t *du)
{
	ksw2amd_pair_t *pp = (ksw2amd_pair_t*)malloc(sizeof(*pp) * (size_t)na);
	ksw_extz_t *ez = (ksw_extz_t*)calloc((size_t)na, sizeof(*ez));
	int32_t *idx = (int32_t*)malloc(sizeof(*idx) * (size_t)na);
	int i, k, rc;
	char msg[96];
	if (!pp || !ez || !idx) { rc = fail(KSW2AMD_E_NOMEM, "local alignment: host allocation failed%s", ""); goto out; }
	for (i = 0, k = 0; i < n; ++i) {
		const ksw2amd_laln_t *a = &aln[i];
		if (a->score <= 0) continue;
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
		rc = ext_batch_scalar(du != 0, km, &sc, na, pp, ez);      /* du: the scalar ksw_extd, the pieces in the caller's order */
	}
	for (k = 0; k < na; ++k) {                 /* the buffers may have grown or moved: always hand them back */
		ksw2amd_laln_t *a = &aln[idx[k]];
		a->cigar = ez[k].cigar; a->m_cigar = ez[k].m_cigar;
		a->n_cigar = rc == KSW2AMD_OK ? ez[k].n_cigar : 0;
	}
	for (k = 0; k < na && rc == KSW2AMD_OK; ++k)
		if (ez[k].score != aln[idx[k]].score) {
			snprintf(msg, sizeof(msg), "%d: local %d, global %d", (int)idx[k], aln[idx[k]].score, ez[k].score);
			rc = fail(KSW2AMD_E_NODEVICE, "local alignment: internal error, the interval's global score differs from the local score on pair %s", msg);
		}
out:
	free(pp); free(ez); free(idx);
	return rc;
}

int lla_align_ex(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln, ll_rev_fn rev,
                 const ll_dual_t *du)
{
	ksw2amd_lres_t *res = 0;
	K2aLLBeg *beg = 0;
	int na = 0, rc;
	/* every argument before anything is staged: the flag here, m / mat / gap costs / pair array / residue codes in ll_batch_ex */
	if (flag & ~LLA_FLAGS) return fail(KSW2AMD_E_PARAM, "local alignment: flag accepts KSW_EZ_SCORE_ONLY, KSW_EZ_RIGHT and KSW_EZ_REV_CIGAR only%s", "");
	if (n > 0 && !aln) return fail(KSW2AMD_E_PARAM, "local alignment: bad pair array%s", "");
	if (n > 0) {
		res = (ksw2amd_lres_t*)malloc(sizeof(*res) * (size_t)n);
		beg = (K2aLLBeg*)malloc(sizeof(*beg) * (size_t)n);
		if (!res || !beg) { rc = fail(KSW2AMD_E_NOMEM, "local alignment: host allocation failed%s", ""); goto out; }
	}
	if ((rc = ll_batch_ex(m, mat, gapo, gape, n, pairs, res, rev, beg, 0, 0, du, 0)) != KSW2AMD_OK) goto out;
	if ((rc = lla_cells(n, res, beg, aln, &na)) != KSW2AMD_OK) goto out;
	if ((flag & KSW_EZ_SCORE_ONLY) || na == 0) goto out;
	rc = lla_cigars(km, m, mat, gapo, gape, flag, n, pairs, 0, na, aln, du);
out:
	free(res); free(beg);
	return rc;
}

int ksw2amd_ll_align_batch(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln)
{
	return lla_align_ex(km, m, mat, gapo, gape, flag, n, pairs, aln, k2a_shim_launch_ll_rev, 0);
}

int ksw2amd_ll_align(void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int flag, ksw2amd_laln_t *aln)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	int rc;
	if (aln) { aln->score = 0; aln->qb = aln->qe = aln->tb = aln->te = -1; aln->n_cigar = 0; }
	if (!p || !aln) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_ll_align: NULL profile or result%s", ""); call_failed("ksw2amd_ll_align", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_ll_align_batch(km, p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, flag, 1, &pr, aln);
	if (rc != KSW2AMD_OK) {
		aln->score = 0; aln->qb = aln->qe = aln->tb = aln->te = -1; aln->n_cigar = 0;
		call_failed("ksw2amd_ll_align", rc, 0);
		return 0;
	}
	return aln->score;
}
