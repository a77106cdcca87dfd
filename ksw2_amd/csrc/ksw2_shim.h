/*
 * ksw2_shim.h -- the thin C-ABI between the C host (ksw2_host_*.c) and the device runtime.
 *
 * The product library links ksw2_shim_hip.hip (HIP runtime + gfx950 kernels).  tests/sim/ links the very
 * same host code against a host-memory, lock-step wave simulator of the same interface so that the
 * packing / scheduling logic can be checked without a GPU; that simulator is test infrastructure and is
 * never part of libksw2_amd.so.
 */
#ifndef KSW2_SHIM_H_
#define KSW2_SHIM_H_

#include <stddef.h>
#include "ksw2_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kernel geometry classes: lanes per alignment (G) x target rows per lane (C) */
#define K2A_NCFG 5
#define K2A_CFG_MP 4      /* generation-serial class: any band, boundary rows through HBM */
static const int k2a_cfg_G[K2A_NCFG] = { 16, 64, 64, 64, 64 };
static const int k2a_cfg_C[K2A_NCFG] = {  8,  8, 16, 32, 16 };
/* geometry classes of the packed-int16 kernels (two same-shape alignments per lane group) */
#ifndef K2A_PKMP_WAVES
#define K2A_PKMP_WAVES 4      /* packed generation-serial class: wavefronts (generations in flight) per task */
#endif
#define K2A_NPKCFG 5
#define K2A_PKCFG_MP 4    /* packed generation-serial class (ksw2_lane_pkmp.h): any band, a workgroup of 4 wavefronts per task */
static const int k2a_pkcfg_G[K2A_NPKCFG] = {  8, 16, 64, 64, 64 };
static const int k2a_pkcfg_C[K2A_NPKCFG] = { 18,  8,  8, 16, 16 };

const char *k2a_shim_backend(void);                /* "hip:gfx950" or "sim" */
const char *k2a_shim_last_error(void);
int   k2a_shim_async_launches(void);         /* 1: launches run on the device behind the call (hip); 0: inside the call (the simulator): what a
                                              * launch waits for on the device must then be complete before the call */
int   k2a_shim_device_count(void);
int   k2a_shim_simd_count(void);               /* SIMDs (wavefront slots side by side) of the current device; 0 = unknown */
int   k2a_shim_set_device(int dev);
int   k2a_shim_pci_bus_id(char *buf, int cap);  /* the current device's directory name under /sys/bus/pci/devices; -1 = unknown */
int   k2a_shim_get_device(void);             /* device of the calling thread; -1 = none */
int   k2a_shim_mem_info(size_t *free_b, size_t *total_b);

/* launch-time kernel forms: every choice the launcher makes can be forced (-1 = automatic, 0 / 1) and is reported */
#define K2A_OPT_LDSCODES 0     /* exact score-only packed (64,16) kernels: target-code planes in LDS */
#define K2A_OPT_LDSROWS  1     /* two-piece traceback packed (64,16) and int32 generation-serial traceback kernels: row state in LDS */
#define K2A_NOPT 2
void  k2a_shim_set_option(int opt, int value);
int   k2a_shim_pk_form(int cfg, int dual, int mode, int nomax, int ntasks);   /* what k2a_shim_launch_fill_pk takes: 0 registers, 1 row state in LDS, 2 code planes in LDS */
int   k2a_shim_mp_form(int dual, int mode, int ntasks);                        /* k2a_shim_launch_fill, class K2A_CFG_MP: 1 = row state in LDS */

void *k2a_shim_malloc(size_t bytes);               /* device memory */
void  k2a_shim_free(void *p);
void *k2a_shim_host_malloc(size_t bytes);          /* pinned host staging */
void  k2a_shim_host_free(void *p);
int   k2a_shim_h2d(void *dst, const void *src, size_t bytes, void *stream);
int   k2a_shim_d2h(void *dst, const void *src, size_t bytes, void *stream);
int   k2a_shim_d2d(void *dst, const void *src, size_t bytes, void *stream);
int   k2a_shim_host_register(void *p, size_t bytes);   /* page-lock caller memory so that uploads from it are asynchronous and at link rate */
int   k2a_shim_host_unregister(void *p);
int   k2a_shim_memset(void *dst, int v, size_t bytes, void *stream);

void *k2a_shim_stream_create(void);
void *k2a_shim_stream_create_high(void);      /* highest priority: hardware queues apart from the ordinary streams' */
void *k2a_shim_stream_create_low(void);       /* lowest priority: the upload streams (copies only), apart from every stream that runs kernels */
void  k2a_shim_stream_destroy(void *stream);
int   k2a_shim_stream_sync(void *stream);
void *k2a_shim_event_create(void);
void  k2a_shim_event_destroy(void *ev);
int   k2a_shim_event_record(void *ev, void *stream);
int   k2a_shim_stream_wait_event(void *stream, void *ev);   /* later work on `stream` waits for `ev` */
float k2a_shim_event_ms(void *start, void *stop);  /* blocks on `stop` */
int   k2a_shim_event_sync(void *ev);               /* blocks until the work recorded before `ev` is done */

/*
 * Fill kernel: ntasks alignments (order[t] = index into pairs/res) on geometry class `cfg`.
 *   dual: 0 single affine gap (extz2 / gg2), 1 two-piece (extd2);  mode: K2A_MODE_*
 * Trace kernel: walks the traceback blocks written by a fill launch of the same class and writes each
 * CIGAR (end -> start order) into cig[pairs[i].cig_off ...], count in res[i].n_cigar.
 */
int k2a_shim_launch_fill(int cfg, int dual, int mode, const K2aScoring *sc, const K2aPair *pairs, const uint32_t *order,
                         int ntasks, const uint8_t *seq, uint8_t *tb, int32_t *bnd, K2aResult *res, void *stream);
int k2a_shim_launch_trace(int cfg, int dual, const K2aPair *pairs, const uint32_t *order, int ntasks, const uint8_t *tb,
                          K2aResult *res, uint32_t *cig, void *stream);

/* Packed-int16 fill: ntasks tasks of TWO same-shape alignments each, order2[2t], order2[2t+1] = their indices (equal
 * for an unpaired leftover); both K2aPair entries point at the task's byte-interleaved sequences and, with
 * mode != SCORE, at the task's shared traceback block (2*C bytes per lane-step).  cfg indexes the k2a_pkcfg_* table.
 * rebased: per-strip score bases (reads of any length whose band window fits 16 bits).
 * nomax: final score and direction bytes only (KSW_EZ_APPROX_MAX launches).
 * The packed trace kernel walks 2*ntasks alignments of such a launch. */
/* defer (exact score-only single-gap classes): the fill tracks row maxima without their columns and streams a checkpoint of every
 * lane's top inputs into `tb`; a second kernel of the same launch call re-runs the strips whose columns the results need
 * (K2aLanePk, DEFER).  Every pair of a wavefront carries the wavefront's checkpoint block in tb_off (byte offset in tb), its
 * stream length in steps in bnd_off and the strips-per-group stride of its header table in cig_off:
 *   block = [bnd_off steps][64 lanes] x 8 bytes, then [64 / G groups][cig_off strips] x 16 bytes (K2aCkHead), then -- G = 64 only,
 *   K2A_FOLD_AFTER -- [cig_off strips] x K2A_CK_REC_WORDS(C) dwords: the strips' records { rmax[C], hl[C] } that the fill folds into
 *   the books behind its step loop (ksw2_lane_pkfold.h).  K2A_CK_BLOCK_BYTES (ksw2_types.h) is the block's size. */
/* qd != NULL (device pointer, K2aQueueDesc in ksw2_types.h): a streamed launch -- the ordinary full grid, every wavefront's task given
 * by its position in the grid, started under the upload: a wavefront first waits (k2a_queue_wait) until the watermark says that the
 * qd->need[] pieces its task lies in have landed, or gives up after the timeout and sets qd->abort; qd->next only counts the
 * wavefront-tasks that started (the fetch compares it with the task count).  Because the grid can fill the device with waiting
 * wavefronts, nothing the pieces depend on may be a kernel queued behind it.  Score-only classes only (mode == K2A_MODE_SCORE):
 * those are what the batch entry points stream. */
int k2a_shim_launch_fill_pk(int cfg, int dual, int mode, int rebased, int nomax, int defer, const K2aScoring *sc, const K2aPair *pairs, const uint32_t *order2,
                            int ntasks, const uint8_t *seq, uint8_t *tb, K2aResult *res, K2aQueueDesc *qd, void *stream);
int k2a_shim_launch_trace_pk(int cfg, int dual, const K2aPair *pairs, const uint32_t *order2, int ntasks, const uint8_t *tb,
                             K2aResult *res, uint32_t *cig, void *stream);

/* uniform plans (K2aUniform, ksw2_types.h): write pairs[n], order2[2 * ntasks] and -- need != NULL -- the streamed launch's
 * need[ceil(ntasks / ng)] on the device */
/* device-resident sources of the exts / extf batch entries: entry k copies len bytes from the device address src to dst + dst_off */
typedef struct K2aGather { uint64_t src; uint32_t dst, len; } K2aGather;
int k2a_shim_launch_gather(const K2aGather *tab, int n, uint8_t *dst, void *stream);
/* 4-bit wire format of uniform plans: bytes / 2 upload bytes at src -> bytes arena bytes at dst (bytes a multiple of 8) */
int k2a_shim_launch_wire_expand(const uint8_t *src, uint8_t *dst, size_t bytes, int fmt, uint32_t stride, void *stream);      /* fmt 1: four bits per code, 2: two bits + escapes */
int k2a_shim_launch_uniform_layout(const K2aUniform *u, K2aPair *pairs, uint32_t *order2, uint32_t *need, void *stream);

/* Packed generation-serial fill (class K2A_PKCFG_MP): one task (two same-shape alignments) per workgroup of four wavefronts that
 * pipeline the task's generations of 1024 target rows.  Both K2aPair entries of a task share bnd_off: K2A_PKMP_BND_WORDS
 * (ksw2_lane_pkmp.h) uint32 of boundary entries followed by K2A_PKMP_WAVES x K2A_PKMP_SPILL_WORDS(16) of row-maximum keys, 16-byte aligned;
 * traceback block as for the int32 generation-serial class but 32 bytes per lane-step.  The packed trace launch with
 * cfg = K2A_PKCFG_MP walks it. */
int k2a_shim_launch_fill_pkmp(int dual, int mode, const K2aScoring *sc, const K2aPair *pairs, const uint32_t *order2, int ntasks,
                              const uint8_t *seq, uint8_t *tb, uint32_t *bnd, K2aResult *res, void *stream);

/* Solo packed fill (ksw2_lane_solo.h): ONE alignment per wavefront using both 16-bit halves (rows [i0,i0+C) and [i0+C,i0+2C) of
 * a double strip), for alignments without a partner of identical shape.  K2A_SOLO_C rows per half; order[t] = pair index. */
#define K2A_SOLO_C 8       /* tasks with a traceback */
/* score-only tasks: 16 rows per half fit the registers (208 VGPRs) and halve the per-step overhead per cell, but 64 lanes x 32
 * rows = 2 048 rows in flight want a band that wide -- at w = 500 half the lanes idle (measured, 1 024 x 10 k x 10 k: 9.5 ms
 * against 7.1 ms with 8 rows, profiles/r3_solo_experiments.txt).  The steps of a task are its columns whatever the height. */
#define K2A_SOLO_CS 8
#define K2A_SOLO_ROWS(score_only) ((score_only) ? K2A_SOLO_CS : K2A_SOLO_C)
int k2a_shim_launch_fill_solo(int dual, int mode, const K2aScoring *sc, const K2aPair *pairs, const uint32_t *order, int ntasks,
                              const uint8_t *seq, uint8_t *tb, K2aResult *res, void *stream);
int k2a_shim_launch_trace_solo(const K2aPair *pairs, const uint32_t *order, int ntasks, const uint8_t *tb, K2aResult *res,
                               uint32_t *cig, void *stream);

/* Splice-aware extension (ksw2_lane_dm.h): one alignment per wavefront, diagonal-major.  pairs[i].bnd_off = dword offset
 * (in seq) of the alignment's packed per-target-position constants, tb_off = its direction bytes ((qlen+tlen-1) rows of
 * min(qlen,tlen) bytes), w / end_bonus set so that k2a_finish applies the plain start-cell rule.  The trace launch walks
 * them with the intron state.  order[t] = index into pairs / res, as for the fill kernels.
 * win = register window class 0 / 1: diagonals up to K2A_DM_DIAG(K2A_DM_SLOTS_S / K2A_DM_SLOTS) cells; win = 2: any length,
 * state in `scratch` (9 * tlen ints per alignment at 4 * pairs[i].pad). */
int k2a_shim_launch_splice_const(const K2aPair *pairs, int n, uint8_t *seq, int noncan, int junc_bonus, void *stream);   /* per-position constants from the uploaded targets */
int k2a_shim_launch_exts(int mode, int win, const K2aSplice *sp, const K2aPair *pairs, const uint32_t *order, int ntasks, const uint8_t *seq,
                         uint8_t *tb, int32_t *scratch, K2aResult *res, void *stream);
int k2a_shim_launch_exts_trace(const K2aSplice *sp, const K2aPair *pairs, const uint32_t *order, int ntasks, const uint8_t *tb,
                               K2aResult *res, uint32_t *cig, void *stream);

/* Gap-linear X-drop extension (ksw2_lane_extf.h): one alignment per wavefront; class 0..2 keep the three state arrays in LDS
 * (targets up to 1024 / 4096 / 21504 residues), class 3 in `scratch` (3 x 16-padded target length bytes at pairs[i].tb_off).
 * Class 4 / 5: register window of 4 / 8 slots, for alignments whose band never holds more than K2A_EXTF_WIN_SPAN(K) positions.
 * pairs[i].zdrop = the X-drop threshold, pairs[i].w the band resolved as in ksw2_extf2_sse.c:23. */
int k2a_shim_launch_extf(int cls, const K2aExtf *par, const K2aPair *pairs, const uint32_t *order, int ntasks, const uint8_t *seq,
                         uint8_t *scratch, K2aResult *res, void *stream);

/* SSE-compatible mode (ksw2_lane_ssec.h): ksw_extz2_sse / ksw_extd2_sse as the reference's SSE kernels return them.  One
 * alignment per wavefront; pairs[i].bnd_off = offset of its state arrays in `scratch` in 16-byte units ((5 or 7) + 4 bytes per
 * 16-padded target position), tb_off = its direction matrix ((qlen + tlen - 1) * k2a_ssec_ncol bytes), pad = K2A_SSEC_* bits,
 * tlen = tlen_full, w = the band resolved as in ksw2_extz2_sse.c:72. */
/* lds_bytes > 0: the tasks' state arrays fit that many bytes each and live in LDS (one wavefront per workgroup) instead of `scratch` */
int k2a_shim_launch_ssec(int dual, int mode, size_t lds_bytes, const K2aSsec *par, const K2aPair *pairs, const uint32_t *order, int ntasks, const uint8_t *seq,
                         uint8_t *tb, uint8_t *scratch, K2aResult *res, void *stream);
int k2a_shim_launch_ssec_blk(int dual, int mode, const K2aSsec *par, const K2aPair *pairs, const uint32_t *order, int ntasks, const uint8_t *seq, uint8_t *tb, K2aResult *res, void *stream);
int k2a_shim_launch_ssec_trace(const K2aPair *pairs, const uint32_t *order, int ntasks, const uint8_t *tb, K2aResult *res, uint32_t *cig, void *stream);

/* Compaction: pool[pos[i] .. pos[i]+res[i].n_cigar) = cig[pairs[i].cig_off ..) for the n pairs of a plan
 * (pos = exclusive prefix sum of n_cigar, computed by the host), so that one D2H brings every CIGAR back. */
int k2a_shim_launch_compact(const K2aPair *pairs, const K2aResult *res, const uint32_t *pos, int n, const uint32_t *cig,
                            uint32_t *pool, void *stream);

/* Local alignment (ksw2_lane_ll.h): one task per wavefront -- an int32 alignment (pk = 0) or two of the same shape in the 16-bit halves
 * (pk = 1; tasks[t].res[1] == res[0]: one alignment in both).  tab = 2 * m * m pen bytes smax - s (rows = target, then rows = query);
 * lds = 0 takes the register column profile (m <= 5).  Row / column codes at seq + roff / coff; tasks over K2A_LL_ROWS rows keep their
 * generation boundary at scratch + boff (8 bytes per column).  res[tasks[t].res[h]] = score, qe, te. */
int k2a_shim_launch_ll(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                       uint8_t *scratch, K2aLLRes *res, void *stream);
/* Start-cell pass of ksw2amd_ll_align_batch, on the SAME task table, tables, sequences and scratch, behind the forward launch in
 * `stream`: half h of a task reads res[tasks[t].res[h]] from device memory and runs the local pass over its reversed prefixes
 * reverse(rows[0 .. re]) x reverse(columns[0 .. ce]); the two halves of a packed task run over their bounding rectangle.
 * beg[tasks[t].res[h]] = that pass's score, qb, tb (score 0: 0, -1, -1, and tasks whose halves both scored 0 leave at once).
 * Only ksw2_host_lla.c calls it (the simulator builds of tests/ll_util.py link the other host objects without it). */
int k2a_shim_launch_ll_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                           uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *stream);
/* The same two launches under the two-piece gap cost of ksw2amd_lld_batch (par->oe2 / ge2): tasks over K2A_LL_ROWS
 * rows keep 16 bytes per column at scratch + tasks[].boff (16-byte aligned).  Packed tasks take the LDS profile whatever `lds` says
 * unless K2A_LLD_PK_REG.  Only ksw2_host_lld.c calls them (the other simulator builds have no such symbols). */
int k2a_shim_launch_lld(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                        uint8_t *scratch, K2aLLRes *res, void *stream);
int k2a_shim_launch_lld_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                            uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *stream);
/* Residue-code check of the flat local-alignment batches (ksw2_lane_llchk.h), launched in `stream` before the chunk's alignment
 * kernels: ent[nent + 1] lists the chunk's distinct sequences (offsets into seq) and numbers their 16-byte blocks, nblocks =
 * ent[nent].first.  *bad, a device word the host set to K2A_LLCHK_NONE, ends up as the lowest ent[].pair with a code >= m.
 * Only ksw2_host_llf.c calls it (the simulator builds of tests/ll_util.py and tests/lla_util.py have no such symbol). */
int k2a_shim_launch_ll_check(const K2aLLChk *ent, int nent, uint32_t nblocks, const uint8_t *seq, int m, uint32_t *bad, void *stream);
/* ksw2amd_ll_sub_batch: the forward launch of k2a_shim_launch_ll on tasks whose rows are the target, writing
 * every task's row profile to prof + 128 * tasks[].pad (K2A_LLSUB_BYTES(nrows) bytes, 16-byte aligned) as well, and behind it in the
 * same stream the reduction: sub[slot] = the largest row maximum outside |t - te| <= d (d = excl, or ceil(score / smax) for excl < 0),
 * the smallest such row, that row's first column.  Only ksw2_host_lls.c calls it (the other simulator builds have no such symbol). */
int k2a_shim_launch_ll_sub(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                           uint8_t *scratch, K2aLLRes *res, uint8_t *prof, int excl, K2aLLSub *sub, void *stream);
/* ksw2amd_lld_sub_batch: the same under the two-piece gap cost -- the forward launch of k2a_shim_launch_lld (16
 * bytes of boundary per column, packed tasks on the LDS profile unless K2A_LLD_PK_REG) that also writes the row profiles, and behind it
 * the reduction of k2a_shim_launch_ll_sub as it is.  Only ksw2_host_llds.c calls it (the other simulator builds have no such symbol). */
int k2a_shim_launch_lld_sub(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                            uint8_t *scratch, K2aLLRes *res, uint8_t *prof, int excl, K2aLLSub *sub, void *stream);
/* ksw2amd_sg_batch: the semi-global mode on the task table of k2a_shim_launch_ll with rows = target
 * (tasks[].swapped = 0) and par->smax = max(0, largest entry): H' = H + gapo + ncols * gape through the same cell update, the free
 * start in the target and the inserted query prefix as boundary values, the maximum over the last column.  res[slot] = (score, ncols - 1,
 * te), the smallest te on a tie.  Only ksw2_host_sg.c and ksw2_host_sga.c call it (the other simulator builds have no such symbol). */
int k2a_shim_launch_sg(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                       uint8_t *scratch, K2aLLRes *res, void *stream);
/* Start pass of ksw2amd_sg_align_batch, on the SAME task table, tables, sequences and scratch, behind
 * k2a_shim_launch_sg in `stream`: half h of a task reads te from res[tasks[t].res[h]] in device memory and aligns the whole reversed query
 * globally against reverse(rows[0 .. te]), anchored at (te, ncols - 1) and free to end in any row.  beg[slot] = (that pass's score, 0, tb):
 * the largest tb at which the score is reached, te + 1 for the empty interval.  Only ksw2_host_sga.c calls it (the other simulator builds
 * have no such symbol). */
int k2a_shim_launch_sg_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                           uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *stream);
/* The same two launches under the two-piece gap cost of ksw2amd_sgd_batch / ksw2amd_sgd_align_batch (par->oe2 / ge2; DESIGN.md section
 * 3.22): the same grids, H' = H + cost(ncols) with cost(l) = min(gapo + l * gape, gapo2 + l * gape2), and 16 bytes of boundary per column
 * at scratch + tasks[].boff (16-byte aligned) for tasks over K2A_LL_ROWS rows.  Packed tasks take the LDS profile whatever `lds` says unless
 * K2A_SGD_PK_REG.  Only ksw2_host_sgd.c calls them (the other simulator builds have no such symbols). */
int k2a_shim_launch_sgd(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                        uint8_t *scratch, K2aLLRes *res, void *stream);
int k2a_shim_launch_sgd_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                            uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *stream);
/* ksw2amd_ov_batch / ksw2amd_ovd_batch: k2a_shim_launch_sg / k2a_shim_launch_sgd with free query ends.  tasks[t].pad
 * holds the task's `ends` (KSW2AMD_OV_QBEG = 1: row -1 is all zeros; KSW2AMD_OV_QEND = 2: the cells of the last target row are candidates
 * beside the last column's); res[slot] = (score, qe, te), the largest H, then the smallest te, then the smallest qe.  A packed task with
 * bit 1 holds a 16-bit column index: ncols <= 65536.  Only ksw2_host_ov.c calls them (the other simulator builds have no such symbols). */
int k2a_shim_launch_ov(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                       uint8_t *scratch, K2aLLRes *res, void *stream);
int k2a_shim_launch_ovd(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                        uint8_t *scratch, K2aLLRes *res, void *stream);
/* The start pass of ksw2amd_ov_align_batch / ksw2amd_ovd_align_batch, behind k2a_shim_launch_ov / k2a_shim_launch_ovd in
 * the stream, on the same task table: half h reads res[slot] = (score, qe, te) and aligns reverse(columns[0 .. qe]) globally against
 * reverse(rows[0 .. te]), anchored at (te, qe), free to end in any row of the last column and, with bit 0 of tasks[t].pad, in any column of
 * the last row.  beg[slot] = (that pass's score, qb, tb): of the cells that reach the score the one with the largest tb, then the largest qb;
 * tb = te + 1 the empty target interval, qb = qe + 1 the empty query interval.  A packed task holds a 16-bit column index: ncols <= 65536.
 * Only ksw2_host_ova.c calls them (the other simulator builds have no such symbols). */
int k2a_shim_launch_ov_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                           uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *stream);
int k2a_shim_launch_ovd_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                            uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *stream);

#ifdef __cplusplus
}
#endif
#endif
