/*
 * ksw2_host_ova.c -- overlap alignment with the start cell and a CIGAR: ksw2amd_ov_align_batch / ksw2amd_ov_align_batch_flat / ksw2amd_ov_align
 * and, under the two-piece gap cost of ksw_extd, ksw2amd_ovd_align_batch / ksw2amd_ovd_align_batch_flat / ksw2amd_ovd_align
 * (include/ksw2_amd.h).  What a caller of ksw2amd_ov_batch does by hand -- reverse query[0..qe] and target[0..te] on the
 * host, an extension call for where the reversed prefixes end, the two corner constants, another call for the CIGAR -- as one call in the three
 * stages of ksw2amd_sg_align_batch (ksw2_host_sga.c):
 *   1. the forward pass of ksw2amd_ov_batch: score, qe, te;
 *   2. the anchored start pass of this mode, launched behind it on what it left in device memory (k2a_shim_launch_ov_rev /
 *      k2a_shim_launch_ovd_rev as the ll_rev_fn): of the start cells (tb, 0) and, with the query's start free, (0, qb) whose global score is
 *      `score`, the one with the largest tb, then the largest qb;
 *   3. the CIGAR of the pairs whose two intervals are non-empty, the scalar-contract ksw_extz (ksw_extd) on query[qb..qe] x target[tb..te];
 *      an empty target interval's (qe + 1) I and an empty query interval's (te + 1) D are written by the host.
 * The stages themselves are sga_align_ex / sga_align_flat_ex, told through ll_fit_t that the mode is overlap and which ends are free.
 *
 * This is the only host object that refers to k2a_shim_launch_ov_rev and k2a_shim_launch_ovd_rev.  The forward launches stay ksw2_host_ov.c's:
 * the mode comes from its ov_mode / ovd_mode.
 */
#include "ksw2_host_int.h"

/* flag and ends before anything is staged (ll_batch_ex checks ends again behind m, mat and the gap costs) */
static int ova_check(const ll_fit_t *ft, int flag)
{
	int rc;
	if ((rc = sga_check_flag(flag)) != KSW2AMD_OK) return rc;
	return ll_ov_check_ends(ft);
}

/* the CIGAR stage of the two-piece entries is the scalar ksw_extd, which returns at once when m <= 1 (ksw2_host_sgd.c, sgd_check_align) */
static int ovda_check(const ll_fit_t *ft, int m, int flag)
{
	int rc;
	if ((rc = ova_check(ft, flag)) != KSW2AMD_OK) return rc;
	if (m == 1) return fail(KSW2AMD_E_PARAM, "overlap alignment: the two-piece align entries need m >= 2 (ksw_extd aligns nothing with m = 1)%s", "");
	return KSW2AMD_OK;
}

int ksw2amd_ov_align_batch(void *km, int m, const int8_t *mat, int gapo, int gape, int ends, int flag, int n, const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln)
{
	ll_fit_t ft;
	int rc;
	ov_mode(&ft, ends);
	if ((rc = ova_check(&ft, flag)) != KSW2AMD_OK) return rc;
	return sga_align_ex(km, m, mat, gapo, gape, flag, n, pairs, aln, &ft, k2a_shim_launch_ov_rev, 0);
}

int ksw2amd_ov_align_batch_flat(void *km, int m, const int8_t *mat, int gapo, int gape, int ends, int flag, int n, const ksw2amd_lflat_t *in, ksw2amd_laln_t *aln)
{
	ll_fit_t ft;
	int rc;
	ov_mode(&ft, ends);
	if ((rc = ova_check(&ft, flag)) != KSW2AMD_OK) return rc;
	return sga_align_flat_ex(km, m, mat, gapo, gape, flag, n, in, aln, &ft, k2a_shim_launch_ov_rev, 0);
}

int ksw2amd_ovd_align_batch(void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int ends, int flag, int n,
                            const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln)
{
	ll_fit_t ft;
	ll_dual_t du;
	int rc;
	ovd_mode(&ft, &du, gapo2, gape2, ends);
	if ((rc = ovda_check(&ft, m, flag)) != KSW2AMD_OK) return rc;
	return sga_align_ex(km, m, mat, gapo, gape, flag, n, pairs, aln, &ft, k2a_shim_launch_ovd_rev, &du);
}

int ksw2amd_ovd_align_batch_flat(void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int ends, int flag, int n,
                                 const ksw2amd_lflat_t *in, ksw2amd_laln_t *aln)
{
	ll_fit_t ft;
	ll_dual_t du;
	int rc;
	ovd_mode(&ft, &du, gapo2, gape2, ends);
	if ((rc = ovda_check(&ft, m, flag)) != KSW2AMD_OK) return rc;
	return sga_align_flat_ex(km, m, mat, gapo, gape, flag, n, in, aln, &ft, k2a_shim_launch_ovd_rev, &du);
}

/* one pair on a ksw_ll_qinit profile: entry 0 of the batch entries, failures reported like ksw_ll_i16 */
int ksw2amd_ov_align(void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int ends, int flag, ksw2amd_laln_t *aln)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	int rc;
	sga_reset(aln ? 1 : 0, aln);
	if (!p || !aln) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_ov_align: NULL profile or result%s", ""); call_failed("ksw2amd_ov_align", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_ov_align_batch(km, p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, ends, flag, 1, &pr, aln);
	if (rc != KSW2AMD_OK) { call_failed("ksw2amd_ov_align", rc, 0); return 0; }
	return aln->score;
}

int ksw2amd_ovd_align(void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int ends, int flag, ksw2amd_laln_t *aln)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	int rc;
	sga_reset(aln ? 1 : 0, aln);
	if (!p || !aln) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_ovd_align: NULL profile or result%s", ""); call_failed("ksw2amd_ovd_align", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_ovd_align_batch(km, p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, gapo2, gape2, ends, flag, 1, &pr, aln);
	if (rc != KSW2AMD_OK) { call_failed("ksw2amd_ovd_align", rc, 0); return 0; }
	return aln->score;
}
