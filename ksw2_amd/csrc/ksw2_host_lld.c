/*
 * ksw2_host_lld.c -- local alignment under the two-piece gap cost of ksw_extd: ksw2amd_lld_batch / ksw2amd_lld_align_batch and their flat
 * forms, and the single-pair entries ksw2amd_lld / ksw2amd_lld_align (include/ksw2_amd.h, DESIGN.md sections 3.18 and 3.19).  A gap of length l costs min(gapo + l * gape, gapo2 + l * gape2), the pieces in the
 * caller's order as in the reference's scalar ksw_extd.  Validation, sort, packed pairing, task table, chunks, the flat entries' check,
 * the result scatter and the CIGAR stage are the single-piece code (ksw2_host_ll.c, ksw2_host_llf.c, ksw2_host_lla.c), told through
 * ll_dual_t what to launch and which second piece to score with.
 *
 * This is the only host object that refers to k2a_shim_launch_lld and k2a_shim_launch_lld_rev (the simulator builds of tests/ll_util.py,
 * tests/lla_util.py, tests/llf_util.py and tests/lls_util.py link the other host objects without them).
 */
#include "ksw2_host_int.h"

static void lld_dual(ll_dual_t *du, int gapo2, int gape2)
{
	du->gapo2 = gapo2; du->gape2 = gape2; du->fwd = k2a_shim_launch_lld; du->pk_reg = K2A_LLD_PK_REG;
}

/* the CIGAR stage is the scalar ksw_extd, which returns at once when m <= 1 (ksw2_extd.c): no alignment to take a CIGAR from */
static int lld_check_align(int m, int flag)
{
	if (flag & ~LLA_FLAGS) return fail(KSW2AMD_E_PARAM, "local alignment: flag accepts KSW_EZ_SCORE_ONLY, KSW_EZ_RIGHT and KSW_EZ_REV_CIGAR only%s", "");
	if (m == 1) return fail(KSW2AMD_E_PARAM, "local alignment: the two-piece align entries need m >= 2 (ksw_extd aligns nothing with m = 1)%s", "");
	return KSW2AMD_OK;
}

int ksw2amd_lld_batch(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res)
{
	ll_dual_t du;
	lld_dual(&du, gapo2, gape2);
	return ll_batch_ex(m, mat, gapo, gape, n, pairs, res, 0, 0, 0, 0, &du, 0);
}

int ksw2amd_lld_batch_flat(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res)
{
	ll_dual_t du;
	lld_dual(&du, gapo2, gape2);
	return llf_batch_ex(m, mat, gapo, gape, n, in, res, 0, 0, 0, 0, &du, 0);
}

int ksw2amd_lld_align_batch(void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int flag, int n, const ksw2amd_lpair_t *pairs,
                            ksw2amd_laln_t *aln)
{
	ll_dual_t du;
	int rc;
	if ((rc = lld_check_align(m, flag)) != KSW2AMD_OK) return rc;
	lld_dual(&du, gapo2, gape2);
	return lla_align_ex(km, m, mat, gapo, gape, flag, n, pairs, aln, k2a_shim_launch_lld_rev, &du);
}

int ksw2amd_lld_align_batch_flat(void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int flag, int n, const ksw2amd_lflat_t *in,
                                 ksw2amd_laln_t *aln)
{
	ll_dual_t du;
	int rc;
	if ((rc = lld_check_align(m, flag)) != KSW2AMD_OK) return rc;
	lld_dual(&du, gapo2, gape2);
	return llf_align_ex(km, m, mat, gapo, gape, flag, n, in, aln, k2a_shim_launch_lld_rev, &du);
}

/* one pair on a ksw_ll_qinit profile: ksw_ll_i16 and ksw2amd_ll_align under the two-piece cost, wrappers over the batch entries above */
int ksw2amd_lld(void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int *qe, int *te)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	ksw2amd_lres_t r;
	int rc;
	if (qe) *qe = -1;
	if (te) *te = -1;
	if (!p) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_lld: NULL profile%s", ""); call_failed("ksw2amd_lld", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_lld_batch(p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, gapo2, gape2, 1, &pr, &r);
	if (rc != KSW2AMD_OK) { call_failed("ksw2amd_lld", rc, 0); return 0; }
	if (qe) *qe = r.qe;
	if (te) *te = r.te;
	return r.score;
}

int ksw2amd_lld_align(void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int flag, ksw2amd_laln_t *aln)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	int rc;
	if (aln) { aln->score = 0; aln->qb = aln->qe = aln->tb = aln->te = -1; aln->n_cigar = 0; }
	if (!p || !aln) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_lld_align: NULL profile or result%s", ""); call_failed("ksw2amd_lld_align", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_lld_align_batch(km, p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, gapo2, gape2, flag, 1, &pr, aln);
	if (rc != KSW2AMD_OK) {
		aln->score = 0; aln->qb = aln->qe = aln->tb = aln->te = -1; aln->n_cigar = 0;
		call_failed("ksw2amd_lld_align", rc, 0);
		return 0;
	}
	return aln->score;
}
