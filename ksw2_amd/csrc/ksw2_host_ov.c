/*
 * ksw2_host_ov.c -- overlap alignment: ksw2amd_ov_batch / ksw2amd_ov_batch_flat / ksw2amd_ov and, under the two-piece gap cost of ksw_extd,
 * ksw2amd_ovd_batch / ksw2amd_ovd_batch_flat / ksw2amd_ovd (include/ksw2_amd.h).  The semi-global entries with the
 * query's ends free as `ends` says: KSW2AMD_OV_QBEG makes row -1 of the matrix all zeros, KSW2AMD_OV_QEND adds the cells of the last target row
 * to the candidates of the last query column.  The kernels are the semi-global ones with both as a per-task mode (ksw2_lane_ll.h, OV).
 * Validation, sort, packed pairing, task table, chunks, the flat entries' check, the corners and the result scatter are ll_chunk's
 * (ksw2_host_ll.c, ksw2_host_llf.c), told through ll_fit_t what to launch, that the mode is overlap and which ends are free, and through
 * ll_dual_t which second piece to score with.
 *
 * This is the only host object that refers to k2a_shim_launch_ov and k2a_shim_launch_ovd (the simulator builds of the other
 * tests/ *_util.py link the other host objects without them); ksw2_host_ova.c takes the mode from ov_mode / ovd_mode here.
 */
#include "ksw2_host_int.h"

/* (shared with ksw2_host_ova.c, which must not name the two launches itself) */
void ov_mode(ll_fit_t *ft, int ends)
{
	ft->launch = k2a_shim_launch_ov; ft->ov = 1; ft->ends = ends;
}

void ovd_mode(ll_fit_t *ft, ll_dual_t *du, int gapo2, int gape2, int ends)
{
	ft->launch = k2a_shim_launch_ovd; ft->ov = 1; ft->ends = ends;
	du->gapo2 = gapo2; du->gape2 = gape2; du->fwd = 0; du->pk_reg = 1;      /* the forward launch is ft->launch; every packed form is built */
}

int ksw2amd_ov_batch(int m, const int8_t *mat, int gapo, int gape, int ends, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res)
{
	ll_fit_t ft;
	ov_mode(&ft, ends);
	return ll_batch_ex(m, mat, gapo, gape, n, pairs, res, 0, 0, 0, 0, 0, &ft);
}

int ksw2amd_ov_batch_flat(int m, const int8_t *mat, int gapo, int gape, int ends, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res)
{
	ll_fit_t ft;
	ov_mode(&ft, ends);
	return llf_batch_ex(m, mat, gapo, gape, n, in, res, 0, 0, 0, 0, 0, &ft);
}

int ksw2amd_ovd_batch(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int ends, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res)
{
	ll_fit_t ft;
	ll_dual_t du;
	ovd_mode(&ft, &du, gapo2, gape2, ends);
	return ll_batch_ex(m, mat, gapo, gape, n, pairs, res, 0, 0, 0, 0, &du, &ft);
}

int ksw2amd_ovd_batch_flat(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int ends, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res)
{
	ll_fit_t ft;
	ll_dual_t du;
	ovd_mode(&ft, &du, gapo2, gape2, ends);
	return llf_batch_ex(m, mat, gapo, gape, n, in, res, 0, 0, 0, 0, &du, &ft);
}

/* one pair on a ksw_ll_qinit profile: row 0 of the batch entries, failures reported like ksw_ll_i16 */
int ksw2amd_ov(void *q, int tlen, const uint8_t *target, int gapo, int gape, int ends, int *qe, int *te)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	ksw2amd_lres_t r;
	int rc;
	if (qe) *qe = -1;
	if (te) *te = -1;
	if (!p) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_ov: NULL profile%s", ""); call_failed("ksw2amd_ov", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_ov_batch(p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, ends, 1, &pr, &r);
	if (rc != KSW2AMD_OK) { call_failed("ksw2amd_ov", rc, 0); return 0; }
	if (qe) *qe = r.qe;
	if (te) *te = r.te;
	return r.score;
}

int ksw2amd_ovd(void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int ends, int *qe, int *te)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	ksw2amd_lres_t r;
	int rc;
	if (qe) *qe = -1;
	if (te) *te = -1;
	if (!p) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_ovd: NULL profile%s", ""); call_failed("ksw2amd_ovd", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_ovd_batch(p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, gapo2, gape2, ends, 1, &pr, &r);
	if (rc != KSW2AMD_OK) { call_failed("ksw2amd_ovd", rc, 0); return 0; }
	if (qe) *qe = r.qe;
	if (te) *te = r.te;
	return r.score;
}
