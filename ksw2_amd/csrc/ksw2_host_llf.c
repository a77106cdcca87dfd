/*
 * ksw2_host_llf.c -- flat local-alignment batches: ksw2amd_ll_batch_flat / ksw2amd_ll_align_batch_flat (include/ksw2_amd.h, DESIGN.md
 * section 3.16).  The sequences stay where the caller has them: one arena in host or device memory, a pair being two offsets and two
 * lengths.  The host never reads a byte of it: a chunk's span is uploaded as it is (host arena) or used in place (device arena), the
 * residue codes are checked by k2a_ll_check_kernel before any alignment kernel of the chunk, and everything else -- sort, packed
 * pairing, task table, launches, result scatter -- is ll_chunk of ksw2_host_ll.c, told that its source is borrowed.
 *
 * This is the only host object that refers to k2a_shim_launch_ll_check (handed to ll_chunk as a function pointer: the simulator
 * builds of tests/ll_util.py and tests/lla_util.py link ksw2_host_ll.c without one).
 */
#include "ksw2_host_int.h"

#define LLF_SPAN_MAX 0xffffffffull     /* K2aLLTask.roff / coff are 32-bit offsets from the start of a chunk's span */

static size_t llf_chunk_bytes(void)
{
	const char *v = ENV(LL_CHUNK_BYTES);
	const long long x = v && *v ? atoll(v) : 0;
	return x > 0 && x < 3000000000ll ? (size_t)x : 3000000000u;
}

/* bytes [*lo, *hi) of the arena that pair i references; 0: both sequences are empty */
static int llf_pair_span(const ksw2amd_lflat_t *in, int i, uint64_t *lo, uint64_t *hi)
{
	const uint64_t ql = (uint64_t)imax(in->qlen[i], 0), tl = (uint64_t)imax(in->tlen[i], 0);
	if (!ql && !tl) return 0;
	*lo = !ql ? in->toff[i] : !tl ? in->qoff[i] : in->qoff[i] < in->toff[i] ? in->qoff[i] : in->toff[i];
	*hi = !ql ? in->toff[i] + tl : !tl ? in->qoff[i] + ql : in->qoff[i] + ql > in->toff[i] + tl ? in->qoff[i] + ql : in->toff[i] + tl;
	return 1;
}

/* ksw2amd_ll_batch_flat (rev = 0, sb = 0), the first two stages of ksw2amd_ll_align_batch_flat, and ksw2amd_ll_sub_batch_flat (sb); du: their
 * two-piece forms, sb with du included */
int llf_batch_ex(int m, const int8_t *mat, int gapo, int gape, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res, ll_rev_fn rev, K2aLLBeg *begs,
                 const ll_sub_t *sb, ksw2amd_lsub_t *subs, const ll_dual_t *du, const ll_fit_t *ft)
{
	const size_t limit = llf_chunk_bytes();
	int i, rc, beg = 0, smax = -128;
	char msg[32];
	if ((rc = ll_check_args(m, mat, gapo, gape)) != KSW2AMD_OK || (du && (rc = ll_check_args(m, mat, du->gapo2, du->gape2)) != KSW2AMD_OK)) return rc;
	if (n < 0 || !in || (n > 0 && (!in->base || !in->qoff || !in->toff || !in->qlen || !in->tlen || !res || (rev && !begs) || (sb && !subs))))
		return fail(KSW2AMD_E_PARAM, "local alignment: bad flat batch arguments%s", "");
	if ((rc = ll_ov_check_ends(ft)) != KSW2AMD_OK) return rc;
	for (i = 0; i < m * m; ++i) smax = imax(smax, mat[i]);
	if (ft) smax = imax(smax, 0);
	for (i = 0; i < n; ++i) {                              /* every argument before anything is uploaded */
		uint64_t lo, hi;
		res[i].score = 0; res[i].qe = res[i].te = -1;       /* a failing chunk leaves the later ones at their reset values */
		if (rev) { begs[i].score = 0; begs[i].qb = begs[i].tb = -1; }
		if (sb) { subs[i].score2 = 0; subs[i].qe2 = subs[i].te2 = -1; }
		if (llf_pair_span(in, i, &lo, &hi) && (hi < lo || hi - lo > LLF_SPAN_MAX)) {
			snprintf(msg, sizeof(msg), "%d", i);
			return fail(KSW2AMD_E_PARAM, "local alignment: pair %s: query and target lie more than 4 GiB apart in the arena", msg);
		}
		if (ft && (rc = ll_sg_check_range(i, in->qlen[i], gapo, gape, du, smax)) != KSW2AMD_OK) return rc;
	}
	if (n == 0) return KSW2AMD_OK;
	if (k2a_shim_device_count() <= 0) return fail(KSW2AMD_E_NODEVICE, "no usable %s device", k2a_shim_backend());      /* the check runs there whatever the matrix */
	while (beg < n) {                                       /* chunks: pairs in order while the span and the bytes stay under the limit */
		ll_src_t src;
		size_t b = 0;
		uint64_t clo = 0, chi = 0;
		int end, any = 0;
		for (end = beg; end < n; ++end) {
			const size_t pb = ll_pair_bytes(in->qlen[end], in->tlen[end], sb != 0, du != 0, ft != 0) + 2 * sizeof(K2aLLChk);
			uint64_t lo, hi, nlo = clo, nhi = chi;
			if (llf_pair_span(in, end, &lo, &hi)) { nlo = any && clo < lo ? clo : lo; nhi = any && chi > hi ? chi : hi; }
			if (end > beg && (b + pb > limit || nhi - nlo > limit || nhi - nlo > LLF_SPAN_MAX || end - beg >= (1 << 22))) break;
			if (nhi > nlo) any = 1;
			clo = nlo; chi = nhi;
			b += pb;
		}
		memset(&src, 0, sizeof(src));
		src.flat = in; src.first = beg; src.lo = clo; src.hi = chi; src.check = k2a_shim_launch_ll_check;
		rc = ll_chunk(m, mat, smax, gapo, gape, end - beg, &src, res + beg, rev, rev ? begs + beg : 0, sb, sb ? subs + beg : 0, du, ft);
		if (rc) return rc;
		beg = end;
	}
	return KSW2AMD_OK;
}

int ksw2amd_ll_batch_flat(int m, const int8_t *mat, int gapo, int gape, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res)
{
	return llf_batch_ex(m, mat, gapo, gape, n, in, res, 0, 0, 0, 0, 0, 0);
}

int llf_align_ex(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lflat_t *in, ksw2amd_laln_t *aln, ll_rev_fn rev,
                 const ll_dual_t *du)
{
	ksw2amd_lres_t *res = 0;
	K2aLLBeg *beg = 0;
	ksw2amd_lpair_t *pp = 0;
	uint8_t *host = 0;
	int i, na = 0, rc;
	if (flag & ~LLA_FLAGS) return fail(KSW2AMD_E_PARAM, "local alignment: flag accepts KSW_EZ_SCORE_ONLY, KSW_EZ_RIGHT and KSW_EZ_REV_CIGAR only%s", "");
	if (n > 0 && !aln) return fail(KSW2AMD_E_PARAM, "local alignment: bad flat batch arguments%s", "");
	if (n > 0) {
		res = (ksw2amd_lres_t*)malloc(sizeof(*res) * (size_t)n);
		beg = (K2aLLBeg*)malloc(sizeof(*beg) * (size_t)n);
		if (!res || !beg) { rc = fail(KSW2AMD_E_NOMEM, "local alignment: host allocation failed%s", ""); goto out; }
	}
	/* stages 1 and 2 on the borrowed arena */
	if ((rc = llf_batch_ex(m, mat, gapo, gape, n, in, res, rev, beg, 0, 0, du, 0)) != KSW2AMD_OK) goto reset;
	if ((rc = lla_cells(n, res, beg, aln, &na)) != KSW2AMD_OK) goto out;
	if ((flag & KSW_EZ_SCORE_ONLY) || na == 0) goto out;
	/* stage 3: the intervals [qoff + qb, qoff + qe] x [toff + tb, toff + te] under the scalar ksw_extz (du: ksw_extd) contract.  Host arena: pointers
	 * into it.  Device arena: the span of the intervals comes back in one copy, then the same pointer path */
	pp = (ksw2amd_lpair_t*)malloc(sizeof(*pp) * (size_t)n);
	if (!pp) { rc = fail(KSW2AMD_E_NOMEM, "local alignment: host allocation failed%s", ""); goto out; }
	if (in->on_device) {
		uint64_t lo = UINT64_MAX, hi = 0;
		void *st = thread_stream();
		for (i = 0; i < n; ++i) {
			const ksw2amd_laln_t *a = &aln[i];
			if (a->score <= 0) continue;
			if (in->qoff[i] + (uint64_t)a->qb < lo) lo = in->qoff[i] + (uint64_t)a->qb;
			if (in->toff[i] + (uint64_t)a->tb < lo) lo = in->toff[i] + (uint64_t)a->tb;
			if (in->qoff[i] + (uint64_t)a->qe + 1 > hi) hi = in->qoff[i] + (uint64_t)a->qe + 1;
			if (in->toff[i] + (uint64_t)a->te + 1 > hi) hi = in->toff[i] + (uint64_t)a->te + 1;
		}
		host = (uint8_t*)malloc((size_t)(hi - lo));
		if (!host) { rc = fail(KSW2AMD_E_NOMEM, "local alignment: host allocation failed%s", ""); goto out; }
		if (!st || k2a_shim_d2h(host, in->base + lo, (size_t)(hi - lo), st) || k2a_shim_stream_sync(st)) { rc = fail(KSW2AMD_E_NODEVICE, "local alignment: %s", k2a_shim_last_error()); goto out; }
		for (i = 0; i < n; ++i) {
			const ksw2amd_laln_t *a = &aln[i];
			pp[i].query = pp[i].target = 0; pp[i].qlen = in->qlen[i]; pp[i].tlen = in->tlen[i];
			if (a->score <= 0) continue;
			pp[i].query = host + (in->qoff[i] + (uint64_t)a->qb - lo); pp[i].target = host + (in->toff[i] + (uint64_t)a->tb - lo);
		}
	} else
		for (i = 0; i < n; ++i) { pp[i].query = in->base + in->qoff[i]; pp[i].target = in->base + in->toff[i]; pp[i].qlen = in->qlen[i]; pp[i].tlen = in->tlen[i]; }
	rc = lla_cigars(km, m, mat, gapo, gape, flag, n, pp, in->on_device != 0, na, aln, du);
	goto out;
reset:
	for (i = 0; aln && i < n; ++i) { aln[i].score = 0; aln[i].qb = aln[i].qe = aln[i].tb = aln[i].te = -1; aln[i].n_cigar = 0; }
out:
	free(res); free(beg); free(pp); free(host);
	return rc;
}

int ksw2amd_ll_align_batch_flat(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lflat_t *in, ksw2amd_laln_t *aln)
{
	return llf_align_ex(km, m, mat, gapo, gape, flag, n, in, aln, k2a_shim_launch_ll_rev, 0);
}
