/*
 * ksw2_host_sg.c -- semi-global alignment: ksw2amd_sg_batch / ksw2amd_sg_batch_flat / ksw2amd_sg (include/ksw2_amd.h, DESIGN.md section
 * 3.20).  The whole query, end to end, against the best-scoring interval of the target: the free start in the target and the inserted
 * query prefix are boundary values, nothing is clamped at 0, and the result is the largest H of the last query column, at the smallest
 * target index.  The kernels are the local family's strip schedule on values biased by gapo + qlen * gape (ksw2_lane_ll.h, FIT).
 * Validation, sort, packed pairing, task table, chunks, the flat entry's check and the result scatter are ll_chunk's (ksw2_host_ll.c,
 * ksw2_host_llf.c), told through ll_fit_t what to launch and that the mode is semi-global.
 *
 * Only this host object and ksw2_host_sga.c (ksw2amd_sg_align_batch, which adds the start of the interval and a CIGAR) refer to
 * k2a_shim_launch_sg (the simulator builds of the other tests/ *_util.py link the other host objects without one).
 */
#include "ksw2_host_int.h"

int ksw2amd_sg_batch(int m, const int8_t *mat, int gapo, int gape, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res)
{
	ll_fit_t ft;
	ft.launch = k2a_shim_launch_sg; ft.ov = ft.ends = 0;
	return ll_batch_ex(m, mat, gapo, gape, n, pairs, res, 0, 0, 0, 0, 0, &ft);
}

int ksw2amd_sg_batch_flat(int m, const int8_t *mat, int gapo, int gape, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res)
{
	ll_fit_t ft;
	ft.launch = k2a_shim_launch_sg; ft.ov = ft.ends = 0;
	return llf_batch_ex(m, mat, gapo, gape, n, in, res, 0, 0, 0, 0, 0, &ft);
}

/* one pair on a ksw_ll_qinit profile: row 0 of ksw2amd_sg_batch, failures reported like ksw_ll_i16 */
int ksw2amd_sg(void *q, int tlen, const uint8_t *target, int gapo, int gape, int *qe, int *te)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	ksw2amd_lres_t r;
	int rc;
	if (qe) *qe = -1;
	if (te) *te = -1;
	if (!p) { rc = fail(KSW2AMD_E_PARAM, "ksw2amd_sg: NULL profile%s", ""); call_failed("ksw2amd_sg", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_sg_batch(p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, 1, &pr, &r);
	if (rc != KSW2AMD_OK) { call_failed("ksw2amd_sg", rc, 0); return 0; }
	if (qe) *qe = r.qe;
	if (te) *te = r.te;
	return r.score;
}
