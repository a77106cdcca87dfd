/*
 * ksw2_host_sgd.c -- semi-global alignment under the two-piece gap cost of ksw_extd: ksw2amd_sgd_batch / ksw2amd_sgd_align_batch, their flat
 * forms and the single-pair entries ksw2amd_sgd / ksw2amd_sgd_align (include/ksw2_amd.h).  A gap of length l costs
 * min(gapo + l * gape, gapo2 + l * gape2), the pieces in the caller's order as in the reference's scalar ksw_extd.  Validation, sort, packed
 * pairing, task table, chunks, the flat entries' check, the corners, the result scatter and the three stages of the align entries are the
 * single-piece code (ksw2_host_ll.c, ksw2_host_llf.c, ksw2_host_sga.c), told through ll_fit_t what to launch and through ll_dual_t which
 * second piece to score with.
 *
 * This is the only host object that refers to k2a_shim_launch_sgd and k2a_shim_launch_sgd_rev (the simulator builds of the other
 * tests/ *_util.py link the other host objects without them).
 */
#include "ksw2_host_int.h"

static void sgd_mode(ll_fit_t *ft, ll_dual_t *du, int gapo2, int gape2)
{
	ft->launch = k2a_shim_launch_sgd; ft->ov = ft->ends = 0;
	du->gapo2 = gapo2; du->gape2 = gape2; du->fwd = 0; du->pk_reg = K2A_SGD_PK_REG;      /* the forward launch is ft->launch */
}

/* the CIGAR stage is the scalar ksw_extd, which returns at once when m <= 1 (ksw2_host_lld.c, lld_check_align) */
static int sgd_check_align(int m, int flag)
{
	int rc;
	if ((rc = sga_check_flag(flag)) != KSW2AMD_OK) return rc;
	if (m == 1) return fail(KSW2AMD_E_PARAM, "semi-global alignment: the two-piece align entries need m >= 2 (ksw_extd aligns nothing with m = 1)%s", "");
	return KSW2AMD_OK;
}

int ksw2amd_sgd_batch(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res)
{
	ll_fit_t ft;
	ll_dual_t du;
	sgd_mode(&ft, &du, gapo2, gape2);
	return ll_batch_ex(m, mat, gapo, gape, n, pairs, res, 0, 0, 0, 0, &du, &ft);
}

int ksw2amd_sgd_batch_flat(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res)
{
	ll_fit_t ft;
	ll_dual_t du;
	sgd_mode(&ft, &du, gapo2, gape2);
	return llf_batch_ex(m, mat, gapo, gape, n, in, res, 0, 0, 0, 0, &du, &ft);
}

int ksw2amd_sgd_align_batch(void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int flag, int n, const ksw2amd_lpair_t *pairs,
                            ksw2amd_laln_t *aln)
{
	ll_fit_t ft;
	ll_dual_t du;
	int rc;
	if ((rc = sgd_check_align(m, flag)) != KSW2AMD_OK) return rc;
	sgd_mode(&ft, &du, gapo2, gape2);
	return sga_align_ex(km, m, mat, gapo, gape, flag, n, pairs, aln, &ft, k2a_shim_launch_sgd_rev, &du);
}

int ksw2amd_sgd_align_batch_flat(void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int flag, int n, const ksw2amd_lflat_t *in,
                                 ksw2amd_laln_t *aln)
{
	ll_fit_t ft;
	ll_dual_t du;
	int rc;
	if ((rc = sgd_check_align(m, flag)) != KSW2AMD_OK) return rc;
	sgd_mode(&ft, &du, gapo2, gape2);
	return sga_align_flat_ex(km, m, mat, gapo, gape, flag, n, in, aln, &ft, k2a_shim_launch_sgd_rev, &du);
}

/* one pair on a ksw_ll_qinit profile: ksw2amd_sg and ksw2amd_sg_align under the two-piece cost, wrappers over the batch entries above */
int ksw2amd_sgd(void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int *qe, int *te)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	ksw2amd_lres_t r;
	int rc;
	if (qe) *qe = -1;
	if (te) *te = -1;
	if (!p) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_sgd: NULL profile%s", ""); call_failed("ksw2amd_sgd", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_sgd_batch(p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, gapo2, gape2, 1, &pr, &r);
	if (rc != KSW2AMD_OK) { call_failed("ksw2amd_sgd", rc, 0); return 0; }
	if (qe) *qe = r.qe;
	if (te) *te = r.te;
	return r.score;
}

int ksw2amd_sgd_align(void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int flag, ksw2amd_laln_t *aln)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	int rc;
	sga_reset(aln ? 1 : 0, aln);
	if (!p || !aln) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_sgd_align: NULL profile or result%s", ""); call_failed("ksw2amd_sgd_align", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_sgd_align_batch(km, p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, gapo2, gape2, flag, 1, &pr, aln);
	if (rc != KSW2AMD_OK) { call_failed("ksw2amd_sgd_align", rc, 0); return 0; }
	return aln->score;
}
