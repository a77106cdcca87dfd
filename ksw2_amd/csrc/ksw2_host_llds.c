/*
 * ksw2_host_llds.c -- suboptimal local score under the two-piece gap cost: ksw2amd_lld_sub_batch / ksw2amd_lld_sub_batch_flat /
 * ksw2amd_lld_sub (include/ksw2_amd.h).  The H matrix is that of ksw2amd_lld_batch (ksw2_host_lld.c), the row
 * profile, the window and the reduction are those of ksw2amd_ll_sub_batch (ksw2_host_lls.c): ll_chunk (ksw2_host_ll.c) is handed both an
 * ll_sub_t and an ll_dual_t, takes the second piece and the 16-byte boundary from the one and the launch from the other.
 *
 * This is the only host object that refers to k2a_shim_launch_lld_sub (the simulator builds of tests/ll_util.py, tests/lla_util.py,
 * tests/llf_util.py, tests/lls_util.py and tests/lld_util.py link the other host objects without one).
 */
#include "ksw2_host_int.h"

/* every argument that ll_batch_ex / llf_batch_ex do not see before them; their own checks (both gap pairs, the arrays, the codes) follow */
static int llds_setup(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int excl, ll_sub_t *sb, ll_dual_t *du)
{
	int rc;
	if ((rc = ll_check_args(m, mat, gapo, gape)) != KSW2AMD_OK || (rc = ll_check_args(m, mat, gapo2, gape2)) != KSW2AMD_OK) return rc;
	if (excl > K2A_LLSUB_EXCL_MAX) return fail(KSW2AMD_E_PARAM, "local alignment: excl must be at most 0x3fffffff%s", "");
	sb->launch = k2a_shim_launch_lld_sub; sb->excl = excl;
	du->gapo2 = gapo2; du->gape2 = gape2; du->fwd = 0; du->pk_reg = K2A_LLD_PK_REG;      /* the forward launch is sb->launch */
	return KSW2AMD_OK;
}

int ksw2amd_lld_sub_batch(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int excl, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res,
                          ksw2amd_lsub_t *sub)
{
	ll_sub_t sb;
	ll_dual_t du;
	int rc;
	if ((rc = llds_setup(m, mat, gapo, gape, gapo2, gape2, excl, &sb, &du)) != KSW2AMD_OK) return rc;
	return ll_batch_ex(m, mat, gapo, gape, n, pairs, res, 0, 0, &sb, sub, &du, 0);
}

int ksw2amd_lld_sub_batch_flat(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int excl, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res,
                               ksw2amd_lsub_t *sub)
{
	ll_sub_t sb;
	ll_dual_t du;
	int rc;
	if ((rc = llds_setup(m, mat, gapo, gape, gapo2, gape2, excl, &sb, &du)) != KSW2AMD_OK) return rc;
	return llf_batch_ex(m, mat, gapo, gape, n, in, res, 0, 0, &sb, sub, &du, 0);
}

int ksw2amd_lld_sub(void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int excl, int *qe, int *te, ksw2amd_lsub_t *sub)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	ksw2amd_lres_t r;
	ksw2amd_lsub_t s;
	int rc;
	if (qe) *qe = -1;
	if (te) *te = -1;
	if (sub) { sub->score2 = 0; sub->qe2 = sub->te2 = -1; }
	if (!p) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_lld_sub: NULL profile%s", ""); call_failed("ksw2amd_lld_sub", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_lld_sub_batch(p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, gapo2, gape2, excl, 1, &pr, &r, &s);
	if (rc != KSW2AMD_OK) { call_failed("ksw2amd_lld_sub", rc, 0); return 0; }
	if (qe) *qe = r.qe;
	if (te) *te = r.te;
	if (sub) *sub = s;
	return r.score;
}
