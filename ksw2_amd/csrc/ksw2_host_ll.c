/*
 * ksw2_host_ll.c -- local alignment (ksw2.h:92-93): ksw_ll_qinit / ksw_ll_i16 and the batch entry ksw2amd_ll_batch.
 *
 * The reference declares the pair and never defines it; the contract is this library's own (include/ksw2_amd.h, DESIGN.md section
 * 3.14): the best Smith-Waterman score over the full matrix, its cell (largest score, then smallest te, then smallest qe), exact int32.
 * Host side of the batch, modelled on the extf batch path: validate every pair, sort, stage every sequence into one pinned arena with
 * the task table and the pen tables, one upload, one launch per kernel form, one 12-byte-per-pair download.  Kernels: ksw2_lane_ll.h.
 *
 * This is the only host object that calls k2a_shim_launch_ll (tests/sim links the other four against a simulator without it).
 * ksw2amd_ll_align_batch (ksw2_host_lla.c) runs its start-cell pass from what a chunk staged here: it hands ll_batch_ex the launch as a
 * function pointer, so this object never refers to k2a_shim_launch_ll_rev (the simulator builds of tests/ll_util.py link it without one).
 * The two-piece entries (ksw2_host_lld.c, ksw2_host_llds.c) hand in their forward, start-cell and profile-writing launches and the second
 * gap pair the same way (ll_dual_t), and the semi-global entries (ksw2_host_sg.c; with the start pass as the ll_rev_fn: ksw2_host_sga.c)
 * their launch and mode (ll_fit_t); the two-piece semi-global entries (ksw2_host_sgd.c) hand in both an ll_fit_t and an ll_dual_t.
 */
#include "ksw2_host_int.h"

/* the packed form is exact while no H + smax exceeds 65535 (ksw2_lane_ll.h).  A local alignment's best score is at most smax per
 * aligned pair of residues, i.e. min(qlen, tlen) * smax, so (min(qlen, tlen) + 1) * smax <= 65535 bounds every H + smax; columns
 * (the shorter length) must also fit the 16-bit column index of the row maxima. */
static int ll_pk_admit(int qlen, int tlen, int smax)
{
	const int64_t mn = imin(qlen, tlen);
	return (mn + 1) * (int64_t)smax <= 65535 && mn <= 65535;
}

/* the semi-global mode runs on H' = H + B, B = gapo + qlen * gape.  A path that ends in column j has at most
 * j + 1 aligned pairs of residues and starts at H(t, -1) = 0, so H(t, j) <= (j + 1) * smax with smax = max(0, largest entry), and the
 * largest value the packed step forms, H'(t - 1, j - 1) + smax, stays within B + qlen * smax + smax.  The packed form is exact while that
 * fits 16 bits: B + (qlen + 1) * smax <= 65535.  (No column index is kept in 16 bits: the maximum is over the last column only.)
 * With smax = 127 and costs (5, 1): 128 * qlen + 132 <= 65535, a query of 510 is packed and one of 511 is not. */
/* du (ksw2amd_sgd_batch): B = cost(qlen), the smaller of the two pieces -- the bound is exact because B is the min */
static int64_t ll_sg_cost(int l, int gapo, int gape, const ll_dual_t *du)
{
	const int64_t a = (int64_t)gapo + (int64_t)l * gape, b = du ? (int64_t)du->gapo2 + (int64_t)l * du->gape2 : a;
	return a < b ? a : b;
}

int ll_sg_pk_admit(int qlen, int gapo, int gape, const ll_dual_t *du, int smax)
{
	return ll_sg_cost(qlen, gapo, gape, du) + ((int64_t)qlen + 1) * smax <= 65535;
}

/* ... and in int32 while gapo + qlen * (gape + smax) + smax <= 0x3fffffff (pair i of the call, for the message); du: cost(qlen) + (qlen + 1) * smax */
int ll_sg_check_range(int i, int qlen, int gapo, int gape, const ll_dual_t *du, int smax)
{
	char msg[32];
	if (qlen <= 0 || ll_sg_cost(qlen, gapo, gape, du) + ((int64_t)qlen + 1) * smax <= 0x3fffffff) return KSW2AMD_OK;
	snprintf(msg, sizeof(msg), "%d", i);
	if (du) return fail(KSW2AMD_E_PARAM, "semi-global alignment: pair %s: cost(qlen) + (qlen + 1) * smax exceeds 0x3fffffff", msg);
	return fail(KSW2AMD_E_PARAM, "semi-global alignment: pair %s: gapo + qlen * (gape + smax) + smax exceeds 0x3fffffff", msg);
}

/* the overlap entries' `ends`: the two bits and nothing else, before anything is staged */
int ll_ov_check_ends(const ll_fit_t *ft)
{
	if (ft && ft->ov && (ft->ends & ~(KSW2AMD_OV_QBEG | KSW2AMD_OV_QEND))) return fail(KSW2AMD_E_PARAM, "overlap alignment: ends must be a combination of KSW2AMD_OV_QBEG and KSW2AMD_OV_QEND%s", "");
	return KSW2AMD_OK;
}

/* a pair's share of a chunk's byte budget: sequences, table entries, results, the generation boundary (8 bytes per column of a task
 * over one generation; dual: 16) and -- sub: rows = target whatever the lengths -- the row profile; fit: rows = target, no profile */
size_t ll_pair_bytes(int qlen, int tlen, int sub, int dual, int fit)
{
	const size_t ql = (size_t)imax(qlen, 0), tl = (size_t)imax(tlen, 0);
	const size_t rows = sub || fit || tl >= ql ? tl : ql, cols = sub || fit || tl >= ql ? ql : tl;
	return rows + cols + 8 + sizeof(K2aLLTask) + sizeof(K2aLLRes) + sizeof(K2aLLBeg) + (rows > K2A_LL_ROWS ? align_up(cols * (dual ? 16 : 8), 256) : 0)
	       + (sub ? align_up(K2A_LLSUB_BYTES(rows), 256) : 0);
}

typedef struct { int32_t rows, cols, sw; uint32_t idx; int64_t cost; } ll_sort_t;      /* sw: rows = the query (part of a packed task's shape) */
static int cmp_shape(const void *a_, const void *b_)
{
	const ll_sort_t *a = (const ll_sort_t*)a_, *b = (const ll_sort_t*)b_;
	if (a->rows != b->rows) return a->rows > b->rows ? -1 : 1;
	if (a->cols != b->cols) return a->cols > b->cols ? -1 : 1;
	if (a->sw != b->sw) return a->sw < b->sw ? -1 : 1;
	return a->idx < b->idx ? -1 : a->idx > b->idx;
}
static int cmp_cost(const void *a_, const void *b_)
{
	const ll_sort_t *a = (const ll_sort_t*)a_, *b = (const ll_sort_t*)b_;
	if (a->cost != b->cost) return a->cost > b->cost ? -1 : 1;
	return a->idx < b->idx ? -1 : a->idx > b->idx;
}

int ll_check_args(int m, const int8_t *mat, int gapo, int gape)
{
	if (m < 1 || m > K2A_MAXM) return fail(KSW2AMD_E_PARAM, "local alignment: m must be 1..127%s", "");
	if (!mat) return fail(KSW2AMD_E_PARAM, "local alignment: mat is NULL%s", "");
	if (gapo < 0 || gapo > 127 || gape < 0 || gape > 127) return fail(KSW2AMD_E_PARAM, "local alignment: gapo and gape must be 0..127%s", "");
	return KSW2AMD_OK;
}

int ll_bad_code(const uint8_t *s, int len, int m)
{
	int i;
	for (i = 0; i < len; ++i) if (s[i] >= m) return 1;
	return 0;
}

static inline int src_qlen(const ll_src_t *s, int i) { return s->flat ? s->flat->qlen[s->first + i] : s->pairs[i].qlen; }
static inline int src_tlen(const ll_src_t *s, int i) { return s->flat ? s->flat->tlen[s->first + i] : s->pairs[i].tlen; }

/* borrowed arenas: the check list of a chunk -- every distinct non-empty (offset, length) once, with the lowest pair that names it
 * (a query shared by all pairs is scanned once).  ent[nent] is left for the sentinel; -1: allocation failed */
static int ll_check_list(const ll_src_t *src, int n, K2aLLChk *ent)
{
	const ksw2amd_lflat_t *f = src->flat;
	size_t cap = 16, x;
	uint32_t *tab;
	int i, h, nent = 0;
	while (cap < 4 * (size_t)n) cap <<= 1;
	if (!(tab = (uint32_t*)calloc(cap, sizeof(uint32_t)))) return -1;
	for (i = 0; i < n; ++i)
		for (h = 0; h < 2; ++h) {
			const int32_t len = h ? f->tlen[src->first + i] : f->qlen[src->first + i];
			const uint64_t off = (h ? f->toff[src->first + i] : f->qoff[src->first + i]) - src->lo;
			if (len <= 0) continue;
			x = (size_t)((off * 0x9e3779b97f4a7c15ull ^ (uint64_t)(uint32_t)len * 0xc2b2ae3d27d4eb4full) >> 20) & (cap - 1);
			while (tab[x] && (ent[tab[x] - 1].off != (uint32_t)off || ent[tab[x] - 1].len != (uint32_t)len)) x = (x + 1) & (cap - 1);
			if (tab[x]) continue;
			ent[nent].off = (uint32_t)off; ent[nent].len = (uint32_t)len; ent[nent].pair = (uint32_t)i; ent[nent].first = 0;
			tab[x] = (uint32_t)++nent;
		}
	free(tab);
	return nent;
}

/* semi-global mode: the pairs of a chunk that launch nothing and still have a result -- a query without a target; free_beg (the overlap
 * entries with the query's start free): nothing of it has to be inserted */
static void ll_fit_corners(const ll_src_t *src, int n, int gapo, int gape, const ll_dual_t *du, int free_beg, ksw2amd_lres_t *res, K2aLLBeg *beg)
{
	int i;
	for (i = 0; i < n; ++i) {
		const int ql = src_qlen(src, i), tl = src_tlen(src, i);
		if (ql > 0 && tl <= 0) {                                 /* the whole query inserted before the target */
			res[i].score = free_beg ? 0 : -(int)ll_sg_cost(ql, gapo, gape, du); res[i].qe = ql - 1; res[i].te = -1;
			if (beg) { beg[i].score = res[i].score; beg[i].qb = free_beg ? ql : 0; beg[i].tb = 0; }      /* (rev: the empty interval, tb = te + 1; free_beg: the whole query hangs over, qb = qe + 1) */
		}
	}
}

/* one chunk: pairs [0, n) of the caller's.  Where the sequences live is all that differs between the two kinds of source:
 *   gathered (src->pairs): validated by the caller, copied once each into the staging arena behind the task table and the pen tables;
 *   borrowed (src->flat):  the chunk's span [lo, hi) of the caller's arena is the kernels' `seq` as it is -- uploaded in one copy
 *     (host arena) or used in place (device arena) -- and the task table, the pen tables and the check list travel in a small buffer
 *     of their own.  The residue codes are checked on the device (src->check) and the result word read before any alignment kernel
 *     is launched; a code >= m ends the chunk with KSW2AMD_E_PARAM and every result at its reset value.
 * rev: the start-cell pass (beg[i] = its score, qb, tb), launched behind the forward pass on the same task table, tables, sequences
 * and results in device memory; one download brings back both arrays.
 * sb (never with rev): ksw2amd_ll_sub_batch -- rows = target for every pair, the forward launch is sb->launch, which also fills a row
 * profile per task (behind the boundaries in the scratch, at 128 * K2aLLTask.pad) and reduces it into K2aLLSub[n] behind K2aLLRes[n]
 * du: the two-piece gap cost of ksw2amd_lld_batch -- the forward launch is du->fwd (rev: the caller's two-piece start-cell launch), the
 * boundary holds 16 bytes per column
 * sb and du together: ksw2amd_lld_sub_batch -- par.oe2 / ge2 and the 16-byte boundary come from du, the forward
 * launch is sb->launch (the caller's two-piece one; du->fwd is not called), rows are the target, and ll_pair_bytes sizes both
 * ft (never with sb or du): ksw2amd_sg_batch -- rows = target for every pair, the forward launch is
 * ft->launch, smax is max(0, largest entry) and may be 0, the packed form is admitted by ll_sg_pk_admit, and a pair without a query or
 * without a target gets its corner result (ll_fit_corners) once the chunk has passed its checks, instead of being skipped
 * ft with rev: ksw2amd_sg_align_batch (ksw2_host_sga.c) -- rev is the caller's anchored start pass; beg[i] = its
 * score, 0, tb (te + 1 for the empty interval), a corner pair's filled in with its result; the trace lines say "sga"
 * ft and du together (never with sb): ksw2amd_sgd_batch and, with rev, ksw2amd_sgd_align_batch (ksw2_host_sgd.c) --
 * the forward launch is ft->launch (du->fwd is not called), par.oe2 / ge2 and the 16-byte boundary come from du, the corners, the packed
 * admission and the range check use cost(qlen) = min of the two pieces; the trace lines say "sgd" / "sgda"
 * ft->ov (never with sb; with and without du): ksw2amd_ov_batch / ksw2amd_ovd_batch (ksw2_host_ov.c) -- the
 * semi-global chunk with ft->ends in every task's pad; a pair whose query end is free is packed only if qlen - 1 fits the packed form's
 * 16-bit column index as well, a query without a target scores 0 if its start is free; the trace line says "ov" / "ovd" and ends
 * ft->ov with rev: ksw2amd_ov_align_batch / ksw2amd_ovd_align_batch (ksw2_host_ova.c) -- rev is the caller's anchored start
 * pass of this mode; beg[i] = its score, qb, tb; its last-row maximum keeps a 16-bit column too, so a pair whose query start is free is packed
 * under the same condition; the trace lines say "ova" / "ovda" */
int ll_chunk(int m, const int8_t *mat, int smax, int gapo, int gape, int n, const ll_src_t *src, ksw2amd_lres_t *res, ll_rev_fn rev, K2aLLBeg *beg,
             const ll_sub_t *sb, ksw2amd_lsub_t *sub, const ll_dual_t *du, const ll_fit_t *ft)
{
	const char *fv = ENV(LL_FORM), *lv = ENV(LL_LDS);
	const int form = fv && *fv ? atoi(fv) : 1;        /* 0: int32 only; 1: packed for same-shape admissible pairs; 2: packed for every admissible pair */
	const int lds = m > 5 || env_flag(lv, 0);
	const ll_fwd_fn fwd = ft ? ft->launch : du ? du->fwd : k2a_shim_launch_ll;
	const char *tn = ft && ft->ov ? (du ? (rev ? "ovda" : "ovd") : rev ? "ova" : "ov") : ft ? (du ? (rev ? "sgda" : "sgd") : rev ? "sga" : "sg") : du ? "lld" : "ll";      /* the trace lines' prefix */
	const int ov_end = ft && ft->ov && ((ft->ends & KSW2AMD_OV_QEND) || (rev && (ft->ends & KSW2AMD_OV_QBEG)));      /* a packed last-row maximum: forward, or the start pass's */
	char ovs[24] = "";
	const ksw2amd_lflat_t *flat = src->flat;
	ll_sort_t *pk = (ll_sort_t*)malloc(sizeof(ll_sort_t) * (2 * (size_t)n + 2)), *i32 = (ll_sort_t*)malloc(sizeof(ll_sort_t) * (size_t)(n + 1));
	K2aLLTask *tk = 0;
	uint8_t *h_arena = 0, *d_arena = 0, *d_scr = 0, *d_span = 0;
	const uint8_t *d_seq = 0;
	K2aLLRes *h_res = 0, *d_res = 0;
	const size_t res_bytes = (sizeof(K2aLLRes) + (rev ? sizeof(K2aLLBeg) : sb ? sizeof(K2aLLSub) : 0)) * (size_t)n;      /* K2aLLRes[n], then K2aLLBeg[n] or K2aLLSub[n] */
	size_t cap_h = 0, cap_d = 0, cap_s = 0, cap_hr = 0, cap_dr = 0, cap_sp = 0;
	int npk = 0, ni32 = 0, ntk_pk = 0, ntk = 0, nent = 0, i, rc = KSW2AMD_OK;
	size_t tab_off, seq_off, chk_off = 0, bad_off = 0, bytes, scr = 0, prof = 0, prof_off = 0;
	void *st = thread_stream();
	if (!pk || !i32) { free(pk); free(i32); return fail(KSW2AMD_E_NOMEM, "local alignment: host allocation failed%s", ""); }
	for (i = 0; i < n; ++i) {
		const int ql = src_qlen(src, i), tl = src_tlen(src, i);
		ll_sort_t s;
		res[i].score = 0; res[i].qe = res[i].te = -1;
		if (rev) { beg[i].score = 0; beg[i].qb = beg[i].tb = -1; }
		if (sb) { sub[i].score2 = 0; sub[i].qe2 = sub[i].te2 = -1; }
		if (ql <= 0 || tl <= 0 || (!ft && smax <= 0)) continue;          /* nothing scores above 0 (ft: a corner result): no launch */
		s.rows = imax(ql, tl); s.cols = imin(ql, tl); s.sw = ql > tl; s.idx = (uint32_t)i;
		if (sb || ft) { s.rows = tl; s.cols = ql; s.sw = 0; }    /* row maxima (ft: the last column) are per target position only if rows = target */
		s.cost = (int64_t)((s.rows + K2A_LL_ROWS - 1) / K2A_LL_ROWS) * (s.cols + 63);
		if (form > 0 && (ft ? ll_sg_pk_admit(ql, gapo, gape, du, smax) && (!ov_end || ql - 1 <= 65535) : ll_pk_admit(ql, tl, smax) && s.cols <= 65535)) pk[npk++] = s;      /* (sb: the query fits the 16-bit column index) */
		else i32[ni32++] = s;
	}
	/* packed tasks: equal shapes (rows, columns, orientation) side by side; with form 1 a pair without a partner of its shape goes to the int32 form */
	qsort(pk, (size_t)npk, sizeof(ll_sort_t), cmp_shape);
	{	/* pairs from the back of the array to its front (entries n + 1 .. 2 n + 1 are free): a task can take two slots for one entry */
		int k = 0, w = 0;
		memmove(pk + n + 1, pk, sizeof(ll_sort_t) * (size_t)npk);
		while (k < npk) {
			const ll_sort_t *a = &pk[n + 1 + k];
			if (k + 1 < npk && a[1].rows == a[0].rows && a[1].cols == a[0].cols && a[1].sw == a[0].sw) { pk[w++] = a[0]; pk[w++] = a[1]; k += 2; }
			else if (form == 2) { pk[w++] = a[0]; pk[w++] = a[0]; k += 1; }
			else { i32[ni32++] = a[0]; k += 1; }
		}
		npk = w;
	}
	ntk_pk = npk / 2;
	qsort(pk, (size_t)ntk_pk, 2 * sizeof(ll_sort_t), cmp_cost);        /* tasks (pairs of entries) longest first */
	qsort(i32, (size_t)ni32, sizeof(ll_sort_t), cmp_cost);
	ntk = ntk_pk + ni32;
	if (ft && ft->ov) snprintf(ovs, sizeof(ovs), " ends=%d", ft->ends);
	if (trace_on()) fprintf(stderr, "[ksw2_amd] %s: pairs=%d pk_tasks=%d int32_tasks=%d profile=%s%s%s%s\n", tn, n, ntk_pk, ni32, lds ? "lds" : "registers", ovs,
	                        !flat ? "" : flat->on_device ? " arena=device" : " arena=host", du && !lds && !du->pk_reg ? " pk_profile=lds" : "");
	if (rev && trace_on()) fprintf(stderr, "[ksw2_amd] %s-rev: pk_tasks=%d int32_tasks=%d profile=%s%s\n", tn, ntk_pk, ni32, lds ? "lds" : "registers",
	                               du && !lds && !du->pk_reg ? " pk_profile=lds" : "");
	if (sb && trace_on()) fprintf(stderr, "[ksw2_amd] %s-sub: pk_tasks=%d int32_tasks=%d profile=%s excl=%d%s\n", tn, ntk_pk, ni32, lds ? "lds" : "registers", sb->excl,
	                              du && !lds && !du->pk_reg ? " pk_profile=lds" : "");
	if (ntk == 0 && !flat) { if (ft) ll_fit_corners(src, n, gapo, gape, du, ft->ov && (ft->ends & KSW2AMD_OV_QBEG), res, rev ? beg : 0); free(pk); free(i32); return KSW2AMD_OK; }         /* a borrowed chunk without tasks still has its codes checked */
	/* gathered: task table | pen tables (rows = target, rows = query) | sequences (rows, then columns, of every pair once)
	 * borrowed: task table | pen tables | check list (2 n + 1 entries at most) | result word of the check */
	tab_off = align_up(sizeof(K2aLLTask) * (size_t)ntk, 256);
	seq_off = tab_off + align_up((size_t)2 * m * m, 256);
	bytes = seq_off;
	if (flat) {
		chk_off = seq_off;
		bad_off = chk_off + align_up(sizeof(K2aLLChk) * (2 * (size_t)n + 1), 256);
		bytes = bad_off + 256;
	} else {
		for (i = 0; i < npk; ++i) if (i % 2 == 0 || pk[i].idx != pk[i - 1].idx) bytes += align_up((size_t)pk[i].rows, 4) + align_up((size_t)pk[i].cols, 4);
		for (i = 0; i < ni32; ++i) bytes += align_up((size_t)i32[i].rows, 4) + align_up((size_t)i32[i].cols, 4);
	}
	h_arena = (uint8_t*)cache_get(BUF_HSEQ, bytes, &cap_h);
	d_arena = (uint8_t*)cache_get(flat ? BUF_PAIRS : BUF_SEQ, bytes, &cap_d);
	h_res = (K2aLLRes*)cache_get(BUF_HRES, res_bytes, &cap_hr);
	d_res = (K2aLLRes*)cache_get(BUF_RES, res_bytes, &cap_dr);
	if (flat && !flat->on_device && src->hi > src->lo) d_span = (uint8_t*)cache_get(BUF_SEQ, (size_t)(src->hi - src->lo), &cap_sp);
	if (!h_arena || !d_arena || !h_res || !d_res || (flat && !flat->on_device && src->hi > src->lo && !d_span)) {
		rc = fail(KSW2AMD_E_NOMEM, "local alignment: buffer allocation failed: %s", k2a_shim_last_error()); goto out;
	}
	d_seq = !flat ? d_arena : flat->on_device ? flat->base + src->lo : d_span;
	tk = (K2aLLTask*)h_arena;
	{
		uint8_t *tab = h_arena + tab_off;
		size_t off = seq_off;
		int t, a, b;
		for (a = 0; a < m; ++a)
			for (b = 0; b < m; ++b) {
				tab[a * m + b] = (uint8_t)(smax - mat[a * m + b]);             /* rows = target: pen(t, q) */
				tab[m * m + a * m + b] = (uint8_t)(smax - mat[b * m + a]);     /* rows = query:  pen(q, t) */
			}
		for (t = 0; t < ntk; ++t) {
			const int is_pk = t < ntk_pk;
			K2aLLTask *k = &tk[t];
			int h;
			memset(k, 0, sizeof(*k));
			for (h = 0; h < (is_pk ? 2 : 1); ++h) {
				const ll_sort_t *s = is_pk ? &pk[2 * t + h] : &i32[t - ntk_pk];
				const int sw = s->sw;                                      /* rows = the longer sequence; the target on equal lengths */
				k->nrows = s->rows; k->ncols = s->cols; k->swapped = sw;
				k->res[h] = s->idx;
				if (h == 1 && s->idx == k->res[0]) { k->roff[1] = k->roff[0]; k->coff[1] = k->coff[0]; continue; }
				if (flat) {                                                /* the chunk's span is below 4 GiB (ksw2_host_llf.c) */
					const uint64_t qo = flat->qoff[src->first + s->idx] - src->lo, to = flat->toff[src->first + s->idx] - src->lo;
					k->roff[h] = (uint32_t)(sw ? qo : to); k->coff[h] = (uint32_t)(sw ? to : qo);
				} else {
					const ksw2amd_lpair_t *p = &src->pairs[s->idx];
					const uint8_t *rs = sw ? p->query : p->target, *cs = sw ? p->target : p->query;
					k->roff[h] = (uint32_t)off; memcpy(h_arena + off, rs, (size_t)s->rows); off += align_up((size_t)s->rows, 4);
					k->coff[h] = (uint32_t)off; memcpy(h_arena + off, cs, (size_t)s->cols); off += align_up((size_t)s->cols, 4);
				}
			}
			if (!is_pk) { k->res[1] = k->res[0]; k->roff[1] = k->roff[0]; k->coff[1] = k->coff[0]; }
			if (k->nrows > K2A_LL_ROWS) { k->boff = scr; scr += align_up((size_t)k->ncols * (du ? 16 : 8), 256); }
			if (ft && ft->ov) k->pad = ft->ends;
			if (sb) { k->pad = (int32_t)(prof / 128); prof += align_up(K2A_LLSUB_BYTES(k->nrows), 256); }
		}
	}
	prof_off = scr; scr += prof;                        /* the row profiles lie behind the boundaries (a chunk stays under 3 GB: pad holds the offset) */
	if (scr) {
		d_scr = (uint8_t*)cache_get(BUF_TB, scr, &cap_s);
		if (!d_scr) { rc = fail(KSW2AMD_E_NOMEM, "local alignment: scratch allocation failed: %s", k2a_shim_last_error()); goto out; }
	}
	if (flat) {
		/* the check: blocks are cut at 16-byte aligned ADDRESSES of the memory the kernel reads (ksw2_lane_llchk.h) */
		K2aLLChk *ent = (K2aLLChk*)(h_arena + chk_off);
		uint32_t *h_bad = (uint32_t*)(h_arena + bad_off);
		uint64_t nblk = 0;
		char msg[32];
		if ((nent = ll_check_list(src, n, ent)) < 0) { rc = fail(KSW2AMD_E_NOMEM, "local alignment: host allocation failed%s", ""); goto out; }
		for (i = 0; i < nent; ++i) { ent[i].first = (uint32_t)nblk; nblk += K2A_LLCHK_BLOCKS((uint32_t)(((uintptr_t)d_seq + ent[i].off) & 15u), ent[i].len); }
		ent[nent].off = ent[nent].len = 0; ent[nent].pair = K2A_LLCHK_NONE; ent[nent].first = (uint32_t)nblk;
		if (nblk > 0xffffffffu) { rc = fail(KSW2AMD_E_PARAM, "local alignment: a chunk's sequences exceed the check's block count%s", ""); goto out; }
		*h_bad = K2A_LLCHK_NONE;
		if (k2a_shim_h2d(d_arena, h_arena, bytes, st)
		    || (d_span && k2a_shim_h2d(d_span, flat->base + src->lo, (size_t)(src->hi - src->lo), st))
		    || src->check((const K2aLLChk*)(d_arena + chk_off), nent, (uint32_t)nblk, d_seq, m, (uint32_t*)(d_arena + bad_off), st)
		    || k2a_shim_d2h(h_bad, d_arena + bad_off, sizeof(uint32_t), st)
		    || k2a_shim_stream_sync(st)) { rc = fail(KSW2AMD_E_NODEVICE, "local alignment: %s", k2a_shim_last_error()); goto out; }
		if (*h_bad != K2A_LLCHK_NONE) {                   /* no alignment kernel has been launched on this chunk */
			snprintf(msg, sizeof(msg), "%d", src->first + (int)*h_bad);
			rc = fail(KSW2AMD_E_PARAM, "local alignment: pair %s: residue code >= m", msg);
			goto out;
		}
		if (ntk == 0) goto done;
	}
	{
		K2aLL par;
		par.m = m; par.smax = smax; par.oe = gapo + gape; par.ge = gape;
		par.oe2 = du ? du->gapo2 + du->gape2 : 0; par.ge2 = du ? du->gape2 : 0;
		if ((!flat && k2a_shim_h2d(d_arena, h_arena, bytes, st))
		    || (!sb && fwd(1, lds, &par, (const K2aLLTask*)d_arena, ntk_pk, d_seq, d_arena + tab_off, d_scr, d_res, st))
		    || (!sb && fwd(0, lds, &par, (const K2aLLTask*)d_arena + ntk_pk, ni32, d_seq, d_arena + tab_off, d_scr, d_res, st))
		    || (sb && sb->launch(1, lds, &par, (const K2aLLTask*)d_arena, ntk_pk, d_seq, d_arena + tab_off, d_scr, d_res, d_scr + prof_off, sb->excl, (K2aLLSub*)(d_res + n), st))
		    || (sb && sb->launch(0, lds, &par, (const K2aLLTask*)d_arena + ntk_pk, ni32, d_seq, d_arena + tab_off, d_scr, d_res, d_scr + prof_off, sb->excl, (K2aLLSub*)(d_res + n), st))
		    || (rev && rev(1, lds, &par, (const K2aLLTask*)d_arena, ntk_pk, d_seq, d_arena + tab_off, d_scr, d_res, (K2aLLBeg*)(d_res + n), st))
		    || (rev && rev(0, lds, &par, (const K2aLLTask*)d_arena + ntk_pk, ni32, d_seq, d_arena + tab_off, d_scr, d_res, (K2aLLBeg*)(d_res + n), st))
		    || k2a_shim_d2h(h_res, d_res, res_bytes, st)
		    || k2a_shim_stream_sync(st)) { rc = fail(KSW2AMD_E_NODEVICE, "local alignment: %s", k2a_shim_last_error()); goto out; }
	}
	for (i = 0; i < npk; ++i) { const K2aLLRes *r = &h_res[pk[i].idx]; res[pk[i].idx].score = r->score; res[pk[i].idx].qe = r->qe; res[pk[i].idx].te = r->te; }
	for (i = 0; i < ni32; ++i) { const K2aLLRes *r = &h_res[i32[i].idx]; res[i32[i].idx].score = r->score; res[i32[i].idx].qe = r->qe; res[i32[i].idx].te = r->te; }
	if (rev) {
		const K2aLLBeg *hb = (const K2aLLBeg*)(h_res + n);
		for (i = 0; i < npk; ++i) beg[pk[i].idx] = hb[pk[i].idx];
		for (i = 0; i < ni32; ++i) beg[i32[i].idx] = hb[i32[i].idx];
	}
	if (sb) {
		const K2aLLSub *hs = (const K2aLLSub*)(h_res + n);
		for (i = 0; i < npk; ++i) memcpy(&sub[pk[i].idx], &hs[pk[i].idx], sizeof(K2aLLSub));       /* ksw2amd_lsub_t is K2aLLSub */
		for (i = 0; i < ni32; ++i) memcpy(&sub[i32[i].idx], &hs[i32[i].idx], sizeof(K2aLLSub));
	}
done:
	if (ft) ll_fit_corners(src, n, gapo, gape, du, ft->ov && (ft->ends & KSW2AMD_OV_QBEG), res, rev ? beg : 0);
out:
	if (d_scr) cache_put(BUF_TB, d_scr, cap_s);
	if (d_span) cache_put(BUF_SEQ, d_span, cap_sp);
	if (h_arena) cache_put(BUF_HSEQ, h_arena, cap_h);
	if (d_arena) cache_put(flat ? BUF_PAIRS : BUF_SEQ, d_arena, cap_d);
	if (h_res) cache_put(BUF_HRES, h_res, cap_hr);
	if (d_res) cache_put(BUF_RES, d_res, cap_dr);
	free(pk); free(i32);
	return rc;
}

/* ksw2amd_ll_batch (rev = 0, sb = 0), the first two stages of ksw2amd_ll_align_batch (ksw2_host_lla.c), and ksw2amd_ll_sub_batch (ksw2_host_lls.c);
 * du: their two-piece forms, sb with du included (ksw2_host_lld.c, ksw2_host_llds.c) */
int ll_batch_ex(int m, const int8_t *mat, int gapo, int gape, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res, ll_rev_fn rev, K2aLLBeg *begs,
                const ll_sub_t *sb, ksw2amd_lsub_t *subs, const ll_dual_t *du, const ll_fit_t *ft)
{
	int i, rc, beg = 0, smax = -128, any = 0;
	if ((rc = ll_check_args(m, mat, gapo, gape)) != KSW2AMD_OK || (du && (rc = ll_check_args(m, mat, du->gapo2, du->gape2)) != KSW2AMD_OK)) return rc;
	if (n < 0 || (n > 0 && (!pairs || !res || (rev && !begs) || (sb && !subs)))) return fail(KSW2AMD_E_PARAM, "local alignment: bad pair array%s", "");
	if ((rc = ll_ov_check_ends(ft)) != KSW2AMD_OK) return rc;
	for (i = 0; i < m * m; ++i) smax = imax(smax, mat[i]);
	if (ft) smax = imax(smax, 0);
	for (i = 0; i < n; ++i) {                              /* every argument before anything runs */
		const ksw2amd_lpair_t *p = &pairs[i];
		char msg[96];
		if ((p->qlen > 0 && !p->query) || (p->tlen > 0 && !p->target)) { snprintf(msg, sizeof(msg), "%d", i); return fail(KSW2AMD_E_PARAM, "local alignment: pair %s: NULL sequence", msg); }
		if (ft && (rc = ll_sg_check_range(i, p->qlen, gapo, gape, du, smax)) != KSW2AMD_OK) return rc;
		if ((p->qlen > 0 && ll_bad_code(p->query, p->qlen, m)) || (p->tlen > 0 && ll_bad_code(p->target, p->tlen, m))) {
			snprintf(msg, sizeof(msg), "%d", i);
			return fail(KSW2AMD_E_PARAM, "local alignment: pair %s: residue code >= m", msg);
		}
		any |= p->qlen > 0 && p->tlen > 0;
	}
	if (n == 0) return KSW2AMD_OK;
	if ((ft ? any : smax > 0) && k2a_shim_device_count() <= 0) return fail(KSW2AMD_E_NODEVICE, "no usable %s device", k2a_shim_backend());
	while (beg < n) {                                       /* chunks of up to ~3 GB of arena + boundary scratch */
		size_t b = 0;
		int end;
		for (end = beg; end < n; ++end) {
			const size_t pb = ll_pair_bytes(pairs[end].qlen, pairs[end].tlen, sb != 0, du != 0, ft != 0);
			if (end > beg && (b + pb > 3000000000u || end - beg >= (1 << 22))) break;
			b += pb;
		}
		{
			ll_src_t src;
			memset(&src, 0, sizeof(src));
			src.pairs = pairs + beg;
			rc = ll_chunk(m, mat, smax, gapo, gape, end - beg, &src, res + beg, rev, rev ? begs + beg : 0, sb, sb ? subs + beg : 0, du, ft);
		}
		if (rc) return rc;
		beg = end;
	}
	return KSW2AMD_OK;
}

int ksw2amd_ll_batch(int m, const int8_t *mat, int gapo, int gape, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res)
{
	return ll_batch_ex(m, mat, gapo, gape, n, pairs, res, 0, 0, 0, 0, 0, 0);
}

/* ---------------------------------------------------------------- ksw_ll_qinit / ksw_ll_i16 (ksw2.h:92-93) */
void *ksw_ll_qinit(void *km, int size, int qlen, const uint8_t *query, int m, const int8_t *mat)
{
	const int ql = imax(qlen, 0);
	ll_prof_t *p;
	if (size != 1 && size != 2) { fail(KSW2AMD_E_PARAM, "ksw_ll_qinit: size must be 1 or 2%s", ""); return 0; }
	if (m < 1 || m > K2A_MAXM || !mat) { fail(KSW2AMD_E_PARAM, "ksw_ll_qinit: m must be 1..127 and mat non-NULL%s", ""); return 0; }
	if (ql > 0 && (!query || ll_bad_code(query, ql, m))) { fail(KSW2AMD_E_PARAM, "ksw_ll_qinit: query NULL or a residue code >= m%s", ""); return 0; }
	p = (ll_prof_t*)km_realloc(km, 0, sizeof(ll_prof_t) + (size_t)ql + (size_t)m * m);
	if (!p) { fail(KSW2AMD_E_NOMEM, "ksw_ll_qinit: allocation failed%s", ""); return 0; }
	p->size = size; p->qlen = qlen; p->m = m; p->pad = 0;
	if (ql > 0) memcpy((uint8_t*)(p + 1), query, (size_t)ql);
	memcpy((uint8_t*)(p + 1) + ql, mat, (size_t)m * m);
	return p;
}

int ksw_ll_i16(void *q, int tlen, const uint8_t *target, int gapo, int gape, int *qe, int *te)
{
	const ll_prof_t *p = (const ll_prof_t*)q;
	ksw2amd_lpair_t pr;
	ksw2amd_lres_t r;
	int rc;
	if (qe) *qe = -1;
	if (te) *te = -1;
	if (!p) { rc = fail(KSW2AMD_E_PARAM, "ksw_ll_i16: NULL profile%s", ""); call_failed("ksw_ll_i16", rc, 0); return 0; }
	pr.query = (const uint8_t*)(p + 1); pr.qlen = p->qlen; pr.target = target; pr.tlen = tlen;
	rc = ksw2amd_ll_batch(p->m, (const int8_t*)(p + 1) + imax(p->qlen, 0), gapo, gape, 1, &pr, &r);
	if (rc != KSW2AMD_OK) { call_failed("ksw_ll_i16", rc, 0); return 0; }
	if (qe) *qe = r.qe;
	if (te) *te = r.te;
	return r.score;
}
