/*
 * ksw2_host_lls.c -- suboptimal local score: ksw2amd_ll_sub_batch / ksw2amd_ll_sub_batch_flat / ksw2amd_ll_sub (include/ksw2_amd.h,
 * DESIGN.md section 3.17).  The forward pass of ksw2amd_ll_batch with rows = target for every pair, every row's maximum and column
 * streamed to a row profile in HBM, and one reduction wavefront per pair that takes the best row outside the window around the best
 * cell.  Validation, sort, packed pairing, task table, chunks, the flat entries' check and the result scatter are ll_chunk's
 * (ksw2_host_ll.c, ksw2_host_llf.c), told through ll_sub_t what to launch.
 *
 * This is the only host object that refers to k2a_shim_launch_ll_sub (the simulator builds of tests/ll_util.py, tests/lla_util.py and
 * tests/llf_util.py link the other host objects without one).
 */
#include "ksw2_host_int.h"

static int lls_check_excl(int excl)
{
	if (excl > K2A_LLSUB_EXCL_MAX) return fail(KSW2AMD_E_PARAM, "local alignment: excl must be at most 0x3fffffff%s", "");
	return KSW2AMD_OK;
}

int ksw2amd_ll_sub_batch(int m, const int8_t *mat, int gapo, int gape, int excl, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res, ksw2amd_lsub_t *sub)
{
	ll_sub_t sb;
	int rc;
	if ((rc = ll_check_args(m, mat, gapo, gape)) != KSW2AMD_OK || (rc = lls_check_excl(excl)) != KSW2AMD_OK) return rc;
	sb.launch = k2a_shim_launch_ll_sub; sb.excl = excl;
	return ll_batch_ex(m, mat, gapo, gape, n, pairs, res, 0, 0, &sb, sub, 0, 0);
}

int ksw2amd_ll_sub_batch_flat(int m, const int8_t *mat, int gapo, int gape, int excl, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res, ksw2amd_lsub_t *sub)
{
	ll_sub_t sb;
	int rc;
	if ((rc = ll_check_args(m, mat, gapo, gape)) != KSW2AMD_OK || (rc = lls_check_excl(excl)) != KSW2AMD_OK) return rc;
	sb.launch = k2a_shim_launch_ll_sub; sb.excl = excl;
	return llf_batch_ex(m, mat, gapo, gape, n, in, res, 0, 0, &sb, sub, 0, 0);
}

int ksw2amd_ll_sub(void *q, int tlen, const uint8_t *target, int gapo, int gape, int excl, int *qe, int *te, ksw2amd_lsub_t *sub)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	ksw2amd_lres_t r;
	ksw2amd_lsub_t s;
	int rc;
	if (qe) *qe = -1;
	if (te) *te = -1;
	if (sub) { sub->score2 = 0; sub->qe2 = sub->te2 = -1; }
	if (!p) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_ll_sub: NULL profile%s", ""); call_failed("ksw2amd_ll_sub", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_ll_sub_batch(p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, excl, 1, &pr, &r, &s);
	if (rc != KSW2AMD_OK) { call_failed("ksw2amd_ll_sub", rc, 0); return 0; }
	if (qe) *qe = r.qe;
	if (te) *te = r.te;
	if (sub) *sub = s;
	return r.score;
}
