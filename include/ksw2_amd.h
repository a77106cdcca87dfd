/*
 * ksw2_amd.h -- C-ABI of libksw2_amd.so: MI355X (gfx950) implementation of ksw2's banded
 * extension / global alignment hot path.
 *
 * Part 1 is the ksw2 calling surface (same symbol names, argument order and meaning, ksw_extz_t layout
 * and CIGAR encoding as the reference's ksw2.h), so a minimap2-style caller that was compiled against
 * the reference header links against this library unchanged.  Part 2 is the batched front-end the
 * reference does not have: thousands of independent (query, target, band) pairs per launch.
 *
 * Result contract: every function evaluates the alignment on the GPU with the exact
 * band |i-j| <= w and the row-wise Z-drop of the reference's scalar ksw_extz / ksw_extd, and returns
 * score / max / max_q / max_t / mqe / mqe_t / mte / mte_q / zdropped / reach_end / CIGAR bit-identical to THOSE.
 * Where the reference's SSE functions differ from their scalar twins, the default results therefore differ from an SSE
 * build's: mte_q (the SSE kernels report it from their 16-padded range: ~94 % of calls), scores at the edge of narrow
 * bands (their 16-position blocks leak), Z-drop (theirs is per anti-diagonal), max_t / max_q on ties, ksw_gg2_sse on
 * narrow bands; two reference bugs are not reproduced (ksw_extd2_sse with e == e2; its first cell when it swaps the
 * gap pieces).  The SSE-compatible mode (KSW2AMD_EZ_SSE_COMPAT, below) returns the SSE functions' own results instead,
 * every field and the CIGAR, and KSW_EZ_APPROX_MAX | KSW_EZ_APPROX_DROP always does.
 * There is no CPU fallback: without a usable gfx950 device the ksw2-named entry points (which return void) reset *ez
 * (score = KSW_NEG_INF, no CIGAR), count the failure (ksw2amd_error_count), keep its message (ksw2amd_last_error) and report it
 * on stderr or through ksw2amd_set_error_handler -- they never abort across the C boundary unless KSW2AMD_ABORT_ON_ERROR=1 asks
 * for it; the ksw2amd_* entry points return a negative code.
 *
 * Reference interface each declaration replaces is cited as (ksw2.h:LINE).
 */
#ifndef KSW2_AMD_H_
#define KSW2_AMD_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ Part 1: the ksw2 surface */
#ifndef KSW2_H_          /* a caller may include the reference's ksw2.h instead: identical ABI */

#define KSW_NEG_INF        (-0x40000000)          /* (ksw2.h:6)  */

#define KSW_EZ_SCORE_ONLY  0x01                   /* (ksw2.h:8)  no CIGAR */
#define KSW_EZ_RIGHT       0x02                   /* (ksw2.h:9)  right-align gaps */
#define KSW_EZ_GENERIC_SC  0x04                   /* (ksw2.h:10) use mat[] for every residue pair */
#define KSW_EZ_APPROX_MAX  0x08                   /* (ksw2.h:11) alone: like the reference only score + corner CIGAR are returned */
#define KSW_EZ_APPROX_DROP 0x10                   /* (ksw2.h:12) with APPROX_MAX: routed to the SSE-compatible kernels, which reproduce the reference's drop heuristic (see KSW2AMD_EZ_SSE_COMPAT below) */
#define KSW_EZ_EXTZ_ONLY   0x40                   /* (ksw2.h:13) extension only */
#define KSW_EZ_REV_CIGAR   0x80                   /* (ksw2.h:14) CIGAR in end->start order */
#define KSW_EZ_SPLICE_FOR   0x100                  /* (ksw2.h:15) exts2: GT..AG signals (forward transcript strand) */
#define KSW_EZ_SPLICE_REV   0x200                  /* (ksw2.h:16) exts2: CT..AC signals (reverse strand) */
#define KSW_EZ_SPLICE_FLANK 0x400                  /* (ksw2.h:17) exts2: half penalty for GT / AG without the preferred flank */
#define KSW_EZ_EQX         0x800                  /* (ksw2.h:18) =/X instead of M (extd2 only) */

#define KSW_CIGAR_MATCH  0                        /* (ksw2.h:22-27) */
#define KSW_CIGAR_INS    1
#define KSW_CIGAR_DEL    2
#define KSW_CIGAR_N_SKIP 3
#define KSW_CIGAR_EQ     7
#define KSW_CIGAR_X      8

/* (ksw2.h:33-42) 56 bytes; cigar[k] = len<<4 | op; the callee reuses and grows `cigar` (capacity
 * m_cigar), the caller zero-initialises the struct once and finally frees `cigar`. */
typedef struct {
	uint32_t max:31, zdropped:1;
	int max_q, max_t;
	int mqe, mqe_t;
	int mte, mte_q;
	int score;
	int m_cigar, n_cigar;
	int reach_end;
	uint32_t *cigar;
} ksw_extz_t;

#endif /* KSW2_H_ */

/* `km`: NULL -> CIGAR memory comes from libc realloc (caller frees with free()); non-NULL -> the
 * caller's kalloc pool: the library calls the process's krealloc(km, ..) (kalloc.h:14), resolved at run time. */

/* (ksw2.h:64-65) single affine gap, replaces ksw_extz2_sse (ksw2_extz2_sse.c:23-304) */
void ksw_extz2_sse(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                   int8_t q, int8_t e, int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez);
/* (ksw2.h:70-71) two-piece affine gap, replaces ksw_extd2_sse (ksw2_extd2_sse.c:34-409) */
void ksw_extd2_sse(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                   int8_t gapo, int8_t gape, int8_t gapo2, int8_t gape2, int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez);
/* (ksw2.h:89-90) global alignment, replace ksw_gg2 (ksw2_gg2.c:4-114) and ksw_gg2_sse (ksw2_gg2_sse.c:11-126).
 * ksw_gg2: all three CIGAR pointers NULL -> score only.  Band that cannot reach the corner
 * (w < |tlen-qlen|): returns KSW_NEG_INF with *n_cigar_ = 0 (undefined in the reference). */
int ksw_gg2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
            int8_t gapo, int8_t gape, int w, int *m_cigar_, int *n_cigar_, uint32_t **cigar_);
int ksw_gg2_sse(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                int8_t gapo, int8_t gape, int w, int *m_cigar_, int *n_cigar_, uint32_t **cigar_);
/* (ksw2.h:61-62, 67-68, 88) the scalar entry points, evaluated by the same GPU kernels
 * (they are the functions whose results define the contract) */
void ksw_extz(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
              int8_t q, int8_t e, int w, int zdrop, int flag, ksw_extz_t *ez);
void ksw_extd(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
              int8_t gapo, int8_t gape, int8_t gapo2, int8_t gape2, int w, int zdrop, int flag, ksw_extz_t *ez);
int ksw_gg(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
           int8_t gapo, int8_t gape, int w, int *m_cigar_, int *n_cigar_, uint32_t **cigar_);
/* multi-ISA builds of the reference export these names under KSW_CPU_DISPATCH
 * (ksw2_extz2_sse.c:16-24, ksw2_extd2_sse.c:25-36); same functions */
void ksw_extz2_sse41(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                     int8_t q, int8_t e, int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez);
void ksw_extz2_sse2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                    int8_t q, int8_t e, int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez);
void ksw_extd2_sse41(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                     int8_t gapo, int8_t gape, int8_t gapo2, int8_t gape2, int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez);
void ksw_extd2_sse2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                    int8_t gapo, int8_t gape, int8_t gapo2, int8_t gape2, int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez);

/* (ksw2.h:73-74) splice-aware extension, replaces ksw_exts2_sse (ksw2_exts2_sse.c:33-415): affine gap (q, e) plus a long
 * target-consuming gap ("intron") with open cost q2, no extension cost, penalty `noncan` at non-canonical donor /
 * acceptor sites (flag KSW_EZ_SPLICE_FOR / _REV / _FLANK), junc[t] bits 1/2 (forward donor/acceptor), 8/4 (reverse)
 * rewarded with junc_bonus.  Unbanded; Z-drop, max and mqe / mte per anti-diagonal exactly like the reference,
 * CIGAR with N for introns.  Bit-exact against the reference's SSE kernel in exact-max mode.
 * Diagonals of up to 960 cells (min(qlen, tlen)) run from registers, longer ones from an HBM-resident state (slower). */
void ksw_exts2_sse(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                   int8_t gapo, int8_t gape, int8_t gapo2, int8_t noncan, int zdrop, int8_t junc_bonus, int flag, const uint8_t *junc, ksw_extz_t *ez);
void ksw_exts2_sse41(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                     int8_t gapo, int8_t gape, int8_t gapo2, int8_t noncan, int zdrop, int8_t junc_bonus, int flag, const uint8_t *junc, ksw_extz_t *ez);
void ksw_exts2_sse2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                    int8_t gapo, int8_t gape, int8_t gapo2, int8_t noncan, int zdrop, int8_t junc_bonus, int flag, const uint8_t *junc, ksw_extz_t *ez);

/* (ksw2.h:76) gap-linear X-drop extension, score only; replaces ksw_extf2_sse (ksw2_extf2_sse.c:11-98): match `mch`,
 * mismatch -|mis|, gap cost e per base, band w (< 0: none), X-drop on the one cell per anti-diagonal the reference follows.
 * Fills ez->max, max_t, max_q, score (when every anti-diagonal ran) and zdropped; the other fields stay reset.  The
 * reference's results depend on the 16-byte blocking of its SSE loops (cells outside the band are updated too and feed
 * the band's edge); reproduced bit for bit for its SSE4.1 build.  Targets up to 21504 residues keep their state in LDS,
 * longer ones in HBM (slower). */
void ksw_extf2_sse(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t mch, int8_t mis, int8_t e, int w, int xdrop,
                   ksw_extz_t *ez);

/* (ksw2.h:92-93) local alignment; the reference declares this pair but never defines it, so the contract is this library's
 * (DESIGN.md section 3.14): the best Smith-Waterman score of the query against the target over the full, unbanded matrix, with
 * s(t, q) = mat[t * m + q] and a gap of length l costing gapo + l * gape.  *qe / *te = 0-based query / target index of the best
 * cell; ties go to the smallest te, then the smallest qe; a best score of 0 (or qlen <= 0, tlen <= 0) returns 0 with *qe = *te = -1.
 * Exact int32 arithmetic: unlike a 16-bit SSE implementation, scores above 32767 do not saturate (the one intended difference from
 * the name).  m 1..127, gapo / gape 0..127, every residue code < m; size (1 or 2) is stored and changes nothing.
 * ksw_ll_qinit returns ONE block from km (NULL: malloc; free with free() / kfree(km, q)) holding copies of query and mat -- the caller
 * may free its buffers afterwards; no device state.  Bad arguments: NULL, ksw2amd_last_error() says why.
 * ksw_ll_i16 on a device failure or a bad argument returns 0 with *qe = *te = -1 and reports like the void entry points above
 * (ksw2amd_error_count, ksw2amd_last_error, the error handler, KSW2AMD_ABORT_ON_ERROR). */
void *ksw_ll_qinit(void *km, int size, int qlen, const uint8_t *query, int m, const int8_t *mat);
int ksw_ll_i16(void *q, int tlen, const uint8_t *target, int gapo, int gape, int *qe, int *te);

/* ------------------------------------------------------------------ Part 2: batched front-end */

/* scoring shared by every pair of a batch (the arguments m, mat, q, e[, q2, e2] of the calls above) */
typedef struct {
	int32_t m;                 /* residue codes 0..m-1, last one is the wildcard (m <= 127) */
	const int8_t *mat;         /* m*m, mat[target*m + query] */
	int8_t q, e, q2, e2;       /* q2/e2 only read by the two-piece (extd) entry points */
} ksw2amd_scoring_t;

/* one alignment = the per-call arguments of ksw_extz2_sse / ksw_extd2_sse */
typedef struct {
	const uint8_t *query, *target;
	int32_t qlen, tlen;
	int32_t w, zdrop, end_bonus, flag;
} ksw2amd_pair_t;

#define KSW2AMD_OK            0
#define KSW2AMD_E_NODEVICE   (-1)      /* no usable gfx950 device / HIP runtime error */
#define KSW2AMD_E_PARAM      (-2)      /* argument outside what this release supports (see last_error) */
#define KSW2AMD_E_NOMEM      (-3)

const char *ksw2amd_last_error(void);  /* message of the calling thread's last failing call */
const char *ksw2amd_backend(void);     /* "hip:gfx950" */
int ksw2amd_device_count(void);
int ksw2amd_set_device(int device);    /* device used by the calling thread's subsequent calls */
/* each thread keeps the device / pinned buffers of its last batch for reuse (allocation costs milliseconds); this returns the
 * calling thread's and those of the library's worker threads */
void ksw2amd_release_cache(void);
/* Devices the batch entry points below shard their work over (process-wide; pairs are independent, so this is host-side
 * sharding without any collective: the library's worker threads -- KSW2AMD_THREADS per device, default 6 -- pull chunks of
 * the batch from a shared counter).  n = 0 (the default): the calling thread's current device only.
 * Replaces nothing in the reference (ksw2.h has no device notion); SURVEY.md section 8b "device selection / multi-GPU inside". */
int ksw2amd_set_devices(int n, const int *devices);
/* The ksw2-named functions return void (ksw2.h:61-76), so a device failure has no return channel.  The failing call returns with
 * *ez reset (ksw2.h:184-189: score = KSW_NEG_INF, no CIGAR), ksw2amd_error_count() goes up, ksw2amd_last_error() holds the message;
 * by default it is also printed on stderr (first occurrences), with a handler installed the handler gets (function name,
 * KSW2AMD_E_* code, message) instead.  KSW2AMD_ABORT_ON_ERROR=1: abort() after the report. */
typedef void (*ksw2amd_error_fn)(const char *func, int code, const char *msg, void *user);
void ksw2amd_set_error_handler(ksw2amd_error_fn fn, void *user);
long ksw2amd_error_count(void);        /* failed ksw2-named calls so far */

/* Opt-in host path for tiny single calls (replaces nothing of the reference; its one-pair-per-call pattern is cli.c:50-132 /
 * README.md:54-87).  A ksw2-named single-pair call costs a launch and two PCIe round trips here, ~0.5 ms whatever its size.  With
 * cells > 0, every such call whose exact band has at most `cells` DP cells is computed on the calling thread by the library's own
 * scalar code instead -- same result contract, bit for bit (tests/test_small_calls.py) -- and ksw2amd_small_call_count() counts
 * them.  Default 0 = never (KSW2AMD_SMALL_CELLS sets the default).  Not a fallback: it is never taken because something failed,
 * the batch entry points never use it, and the device is initialised by the first call all the same.  KSW_EZ_APPROX_MAX requests
 * and the SSE-compatible mode always go to the device.  Measured crossover and rates: INTEGRATION.md. */
void ksw2amd_set_small_call_cells(int64_t cells);
long ksw2amd_small_call_count(void);
/* diagnostics: { batches run on the worker pool, chunks they were cut into, single-pair calls that were coalesced with other
 * threads' calls, device batches those formed } since the library was loaded */
void ksw2amd_host_stats(int64_t out[4]);
/* where the batch entry points' host threads spent their time, in microseconds summed over threads since the library was loaded:
 * { plan creation (pack / gather into page-locked staging, uploads issued), launch calls, waiting for the device + fetch + ksw_extz_t
 * assembly, plans run }.  For a multi-rank job's per-rank report (bench.py config.per_rank): which side a slow rank was slow on. */
void ksw2amd_host_phase_us(int64_t out[4]);

/* n independent alignments; ez[i] ends up exactly as after
 *   ksw_extz2_sse(km, pairs[i].qlen, pairs[i].query, ..., sc->m, sc->mat, sc->q, sc->e, w, zdrop, end_bonus, flag, &ez[i])
 * (resp. ksw_extd2_sse).  ez[] must be zero-initialised (or hold reusable cigar buffers) like for the
 * single calls.  Large batches are split internally to fit device memory. */
int ksw2amd_extz_batch(void *km, const ksw2amd_scoring_t *sc, int n, const ksw2amd_pair_t *pairs, ksw_extz_t *ez);
int ksw2amd_extd_batch(void *km, const ksw2amd_scoring_t *sc, int n, const ksw2amd_pair_t *pairs, ksw_extz_t *ez);

/* Flat batches (new; no reference counterpart): every sequence of the batch lies in ONE arena and a pair is two offsets and two
 * lengths -- what a caller that reads its sequences into a buffer has anyway.  The library then uploads the arena's span as it
 * is (one copy instead of 2 n gathers into staging; asynchronous and at link rate if the arena is page-locked, ksw2amd_host_register)
 * and never walks over the bytes on the host: a pair with a wildcard code in a packed-int16 kernel is reported by the kernel
 * and run again through the int32 kernels.  `on_device` != 0: `base` is device memory (a hipMalloc'ed arena of the calling
 * thread's device, e.g. a shard that RCCL delivered): no upload at all (pairs that ask for the SSE kernels' own results, which keep
 * their state on the host side of the plan, have the arena's span brought back first).  Per-pair arrays w / zdrop / end_bonus / flag may be NULL:
 * the *_all value then applies to every pair.  Results are those of the ordinary entry points on the same pairs. */
typedef struct {
	const uint8_t *base;                  /* the arena */
	const uint64_t *qoff, *toff;          /* [n] byte offsets of query / target in the arena (one plan spans at most 4 GiB of it) */
	const int32_t *qlen, *tlen;           /* [n] */
	const int32_t *w, *zdrop, *end_bonus, *flag;      /* [n] or NULL */
	int32_t w_all, zdrop_all, end_bonus_all, flag_all;
	int32_t on_device;
} ksw2amd_flat_t;
int ksw2amd_extz_batch_flat(void *km, const ksw2amd_scoring_t *sc, int n, const ksw2amd_flat_t *in, ksw_extz_t *ez);
int ksw2amd_extd_batch_flat(void *km, const ksw2amd_scoring_t *sc, int n, const ksw2amd_flat_t *in, ksw_extz_t *ez);
/* device memory of the calling thread's device for a device-resident arena, without linking the HIP runtime (synchronous copies) */
void *ksw2amd_device_alloc(size_t bytes);
void  ksw2amd_device_free(void *d);
int   ksw2amd_device_upload(void *dst, const void *src, size_t bytes);
int   ksw2amd_device_download(void *dst, const void *src, size_t bytes);
/* page-lock / release caller memory (an arena that is reused from batch to batch): uploads from it need no staging copy */
int ksw2amd_host_register(const void *p, size_t bytes);
int ksw2amd_host_unregister(const void *p);

/* SSE-compatible mode (opt-in).  By default the "...2_sse" functions above return the exact-band, row-wise results of the
 * scalar ksw_extz / ksw_extd (the contract).  The reference's SSE kernels differ from that where their
 * 16-position blocks leak across the band edge, in their anti-diagonal Z-drop, in mte_q, in tie order.  A
 * caller that must reproduce an SSE build's output bit for bit -- every ksw_extz_t field and the CIGAR -- asks for it
 *   per pair:      KSW2AMD_EZ_SSE_COMPAT or-ed into the flags of the single calls / of ksw2amd_pair_t, or
 *   process-wide:  ksw2amd_set_sse_compat(1), or KSW2AMD_SSE_COMPAT=1 in the environment of an unchanged caller.
 * Those pairs run through kernels that keep the SSE data flow (ksw2_extz2_sse.c:101-301, ksw2_extd2_sse.c:131-398; one
 * alignment per wavefront, slower than the default path).  KSW_EZ_APPROX_MAX | KSW_EZ_APPROX_DROP always takes this path:
 * that heuristic is defined by the SSE data flow (KSW2AMD_APPROX_DROP_EXACT=1 computes exactly instead). */
#define KSW2AMD_EZ_SSE_COMPAT 0x20000000
void ksw2amd_set_sse_compat(int on);

/* splice-aware batches: the arguments of ksw_exts2_sse, scoring shared by the batch */
typedef struct {
	int32_t m;
	const int8_t *mat;
	int8_t q, e, q2, noncan, junc_bonus;
} ksw2amd_splice_t;
typedef struct {
	const uint8_t *query, *target, *junc;        /* junc may be NULL */
	int32_t qlen, tlen;
	int32_t zdrop, flag;
} ksw2amd_spair_t;
int ksw2amd_exts_batch(void *km, const ksw2amd_splice_t *sc, int n, const ksw2amd_spair_t *pairs, ksw_extz_t *ez);

/* gap-linear X-drop batches: the arguments of ksw_extf2_sse, scoring shared by the batch.  ez[i] ends up exactly as after
 *   ksw_extf2_sse(km, pairs[i].qlen, pairs[i].query, pairs[i].tlen, pairs[i].target, mch, mis, e, pairs[i].w, pairs[i].xdrop, &ez[i]) */
typedef struct {
	const uint8_t *query, *target;
	int32_t qlen, tlen;
	int32_t w, xdrop;
} ksw2amd_fpair_t;
int ksw2amd_extf_batch(void *km, int8_t mch, int8_t mis, int8_t e, int n, const ksw2amd_fpair_t *pairs, ksw_extz_t *ez);
/* The same two with the sequences (and junction arrays) in DEVICE memory: pairs[].query / target / junc are device pointers -- a
 * shard of a multi-GPU job that RCCL delivered into HBM (ksw2_amd/parallel.py).  One kernel gathers them into the plan's arena;
 * nothing of them crosses the link.  (Replaces nothing in the reference: ksw2.h has no notion of a device.) */
int ksw2amd_exts_batch_device(void *km, const ksw2amd_splice_t *sc, int n, const ksw2amd_spair_t *pairs, ksw_extz_t *ez);
int ksw2amd_extf_batch_device(void *km, int8_t mch, int8_t mis, int8_t e, int n, const ksw2amd_fpair_t *pairs, ksw_extz_t *ez);

/* local-alignment batches (ksw_ll_i16 above, many pairs per launch): res[i] is what
 *   ksw_ll_i16(ksw_ll_qinit(0, 2, pairs[i].qlen, pairs[i].query, m, mat), pairs[i].tlen, pairs[i].target, gapo, gape, &qe, &te)
 * returns (score, qe, te).  Every argument and every residue code is checked before anything runs: KSW2AMD_E_PARAM, no launch.
 * Pairs of the same shape whose best score provably fits 16 bits run two per wavefront in packed 16-bit arithmetic, the others in
 * int32; the results are the same. */
typedef struct {
	const uint8_t *query, *target;
	int32_t qlen, tlen;
} ksw2amd_lpair_t;
typedef struct {
	int32_t score, qe, te;
} ksw2amd_lres_t;
int ksw2amd_ll_batch(int m, const int8_t *mat, int gapo, int gape, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res);

/* Local alignment with start cell and CIGAR (new; what a caller of ksw_ll_i16 does next by hand -- reverse both prefixes, a second
 * pass for the start, a global alignment of the interval -- as one call).  For every pair:
 *   score, qe, te   exactly what ksw2amd_ll_batch returns;
 *   qb, tb          with (s', qe', te') = ksw2amd_ll_batch's result on reverse(query[0..qe]), reverse(target[0..te]): qb = qe - qe',
 *                   tb = te - te' (s' == score always).  In words: among the start cells of the best-scoring alignments that end in
 *                   (qe, te), the largest tb, then the largest qb.  The alignment covers query[qb..qe] and target[tb..te], inclusive;
 *   cigar           exactly the CIGAR of the scalar ksw_extz(km, qe-qb+1, query+qb, te-tb+1, target+tb, m, mat, gapo, gape, -1, -1,
 *                   KSW_EZ_GENERIC_SC | (flag & (KSW_EZ_RIGHT | KSW_EZ_REV_CIGAR)), &ez), whose global score equals `score` (checked
 *                   for every pair; a mismatch is reported as an error, never returned).  With gapo + gape > 0 it begins and ends with M.
 * flag: KSW_EZ_SCORE_ONLY (coordinates only, n_cigar = 0, no third stage), KSW_EZ_RIGHT, KSW_EZ_REV_CIGAR; any other bit is
 * KSW2AMD_E_PARAM.  A best score of 0 (an empty sequence, a matrix without a positive entry): score = 0, qb = qe = tb = te = -1,
 * n_cigar = 0, nothing launched for the pair.  Arguments as for ksw2amd_ll_batch (m 1..127, gapo / gape 0..127, every residue code
 * < m), all checked before anything is staged or launched.  The start-cell pass runs on the device from what the forward pass left
 * there (no download, host reversal or second upload in between).  aln[] is zero-initialised by the caller or holds reusable CIGAR
 * buffers (cigar / m_cigar, grown through km like ksw_extz_t.cigar).  Device failures: a negative code, no CPU fallback. */
typedef struct {
	int32_t score;              /* as ksw2amd_ll_batch */
	int32_t qb, qe, tb, te;     /* 0-based, inclusive */
	int32_t m_cigar, n_cigar;
	uint32_t *cigar;            /* len<<4 | op */
} ksw2amd_laln_t;
int ksw2amd_ll_align_batch(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln);
/* one pair, on a profile from ksw_ll_qinit; returns the score.  On a device failure or a bad argument it returns 0 with the four
 * coordinates -1 and n_cigar = 0, and reports like ksw_ll_i16 */
int ksw2amd_ll_align(void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int flag, ksw2amd_laln_t *aln);

/* Flat local-alignment batches (new): every sequence lies in ONE arena -- host memory, or device memory of
 * the calling thread's device -- and a pair is two offsets and two lengths.  res[i] / aln[i] are exactly what ksw2amd_ll_batch /
 * ksw2amd_ll_align_batch return for the pair (base + qoff[i], qlen[i], base + toff[i], tlen[i]): tie rules, the (0, -1, -1) results,
 * CIGAR buffer reuse through km and the flags included.  Offsets need no alignment; sequences may overlap or be shared between pairs
 * (one query against many targets is one copy of the query).
 * The library never walks over the arena's bytes on the host.  Host arena: the span of the arena that a chunk's pairs reference goes
 * up as it is, in one copy, bytes between the sequences included (asynchronous and without staging when the arena is page-locked,
 * ksw2amd_host_register).  Device arena (on_device != 0): nothing crosses the link for the two kernel passes; the CIGAR stage of
 * ksw2amd_ll_align_batch_flat brings the span of the aligned intervals back to the host once.
 * m, mat, the gap costs, NULL arrays, a negative n and the flag bits are checked on the host before anything is uploaded.  Residue
 * codes are checked ON THE DEVICE, chunk by chunk, before any alignment kernel of the chunk is launched (only the bytes of referenced
 * sequences: a byte >= m between two sequences is not an error).  A code >= m: KSW2AMD_E_PARAM, ksw2amd_last_error() names the lowest
 * offending pair of that chunk, no alignment kernel has run on the chunk, and the entries of that chunk and of every later one hold
 * the reset values (score 0, coordinates -1, n_cigar 0).  Large batches are cut into chunks (pairs in order; about 3 GB of sequence, or
 * KSW2AMD_LL_CHUNK_BYTES when that is lower): res[] of EARLIER chunks of such a call may already hold results when a later chunk fails
 * (ksw2amd_ll_align_batch_flat resets every entry).  Limit: the task table addresses a chunk's span with 32 bits, so the two
 * sequences of ONE pair must lie within 4 GiB of each other in the arena (KSW2AMD_E_PARAM otherwise); pairs may lie anywhere. */
typedef struct {
	const uint8_t *base;            /* the arena: host memory, or device memory of the calling thread's device */
	const uint64_t *qoff, *toff;    /* [n] byte offsets; any alignment; sequences may overlap or be shared between pairs */
	const int32_t *qlen, *tlen;     /* [n] */
	int32_t on_device;
} ksw2amd_lflat_t;
int ksw2amd_ll_batch_flat(int m, const int8_t *mat, int gapo, int gape, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res);
int ksw2amd_ll_align_batch_flat(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n, const ksw2amd_lflat_t *in, ksw2amd_laln_t *aln);

/* Suboptimal local score (new): the member of the classic local-alignment record that BWA's
 * ksw_align reports as kswr_t.score2 / te2 and SSW as score2 / ref_end2 -- the second-best score OUTSIDE the neighbourhood of the best
 * hit, from which a caller derives a mapping quality or a repeat call.  With H(t, j) the matrix of ksw2amd_ll_batch (t: target index,
 * j: query index), (score, qe, te) its result and R(t) = max_j H(t, j) the maximum of target row t:
 *   d       = excl when excl >= 0, else ceil(score / smax), smax the largest matrix entry (BWA's default: an alignment that scores
 *             `score` spans at least that many target rows); the rows with |t - te| <= d are excluded;
 *   score2  = the largest R(t) over the rows that are not excluded;
 *   te2     = the smallest such t that attains it;   qe2 = the smallest j with H(te2, j) == score2;
 *   score2 == 0 (every row excluded, no positive cell outside the window, or score == 0): te2 = qe2 = -1.
 * It is the plain maximum over rows: runs of adjacent rows are NOT merged into "peaks" as BWA does before it compares them, so a
 * shoulder of the best alignment that reaches beyond the window counts.  res[i] is bit for bit what ksw2amd_ll_batch returns.
 * Arguments as for ksw2amd_ll_batch (m 1..127, gapo / gape 0..127, every residue code < m) and excl <= 0x3fffffff, all checked before
 * anything is launched: KSW2AMD_E_PARAM.  The flat entry takes an arena like ksw2amd_ll_batch_flat, with the same check on the device,
 * the same chunks and the same error semantics; sub[] is reset together with res[].  Pairs that never reach the device (an empty
 * sequence, a matrix without a positive entry) get (0, -1, -1).  ksw2amd_ll_align_batch does not carry the suboptimal score: compute
 * it for all pairs here and ask for start and CIGAR on those you keep.  Cost: target rows are the matrix rows whatever the lengths, so
 * a target much shorter than its query fills few lanes of a wavefront (ksw2amd_ll_batch would have turned the pair round). */
typedef struct {
	int32_t score2, qe2, te2;
} ksw2amd_lsub_t;
int ksw2amd_ll_sub_batch(int m, const int8_t *mat, int gapo, int gape, int excl, int n,
                         const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res, ksw2amd_lsub_t *sub);
int ksw2amd_ll_sub_batch_flat(int m, const int8_t *mat, int gapo, int gape, int excl, int n,
                              const ksw2amd_lflat_t *in, ksw2amd_lres_t *res, ksw2amd_lsub_t *sub);
/* one pair on a ksw_ll_qinit profile; returns the score.  On a device failure or a bad argument it returns 0 with *qe = *te = -1 and
 * *sub = (0, -1, -1), and reports like ksw_ll_i16 */
int ksw2amd_ll_sub(void *q, int tlen, const uint8_t *target, int gapo, int gape, int excl,
                   int *qe, int *te, ksw2amd_lsub_t *sub);

/* Local alignment under the two-piece gap cost of ksw_extd (new): the four batch entries above
 * with a gap of length l costing min(gapo + l * gape, gapo2 + l * gape2) -- the cost of the reference's scalar ksw_extd, which never swaps
 * or orders the two pieces, and neither does this.  H(i,j) = max(0, H(i-1,j-1) + s, E, F, E2, F2) over the full matrix in exact int32
 * arithmetic; (score, qe, te), the tie rule, the (0, -1, -1) result, qb / tb from the pass over the reversed prefixes (s' == score is
 * checked for every pair) as for ksw2amd_ll_batch / ksw2amd_ll_align_batch.  cigar is exactly that of the scalar
 *   ksw_extd(km, qe-qb+1, query+qb, te-tb+1, target+tb, m, mat, gapo, gape, gapo2, gape2, -1, -1, flag & (KSW_EZ_RIGHT | KSW_EZ_REV_CIGAR), &ez)
 * whose global score equals `score` (checked for every pair; a mismatch is an error, never returned); it begins and ends with M when
 * min(gapo + gape, gapo2 + gape2) > 0.  With (gapo2, gape2) = (gapo, gape), or gapo2 >= gapo and gape2 >= gape, every result equals
 * the single-piece entry's.  Arguments: m 1..127, all four gap costs 0..127, every residue code < m; flag as for
 * ksw2amd_ll_align_batch; all checked before anything is staged or launched (flat entries: the codes on the device, chunk by chunk).
 * One corner is rejected up front with KSW2AMD_E_PARAM: the two align entries with m = 1, whatever the flag (the scalar ksw_extd aligns
 * nothing when m <= 1, so there is no CIGAR contract to meet; ksw2amd_lld_batch / _flat accept m = 1).  The flat entries carry the chunking,
 * the on-device code check, the reset and error semantics and the on_device behaviour of ksw2amd_ll_batch_flat /
 * ksw2amd_ll_align_batch_flat unchanged.  Device failures: a negative code, no CPU fallback.  KSW2AMD_LL_FORM / KSW2AMD_LL_CHUNK_BYTES
 * govern these entries too; KSW2AMD_LL_LDS only their int32 tasks (packed two-piece tasks always read scores from LDS).
 * The two-piece suboptimal score and the single-pair entries on a ksw_ll_qinit profile follow the four batch entries. */
int ksw2amd_lld_batch(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res);
int ksw2amd_lld_align_batch(void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int flag, int n, const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln);
int ksw2amd_lld_batch_flat(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res);
int ksw2amd_lld_align_batch_flat(void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int flag, int n, const ksw2amd_lflat_t *in, ksw2amd_laln_t *aln);

/* Suboptimal local score under the two-piece gap cost, and the two-piece single-pair entries (new).
 * With H the matrix of ksw2amd_lld_batch -- max(0, diag + s, E, F, E2, F2), exact int32 -- res[i] is bit for bit what ksw2amd_lld_batch
 * returns, and R(t), d, score2, te2, qe2 and the (0, -1, -1) cases are those of ksw2amd_ll_sub_batch read on this H: d = excl when
 * excl >= 0, else ceil(score / smax) with the two-piece score.  With (gapo2, gape2) = (gapo, gape), or gapo2 >= gapo and gape2 >= gape,
 * every result equals ksw2amd_ll_sub_batch's.  Arguments: m 1..127 (m = 1 is accepted), all four gap costs 0..127, excl <= 0x3fffffff,
 * every residue code < m, all checked before anything is launched (KSW2AMD_E_PARAM); the flat entry checks the codes on the device, chunk
 * by chunk, and has the chunking, reset and error semantics of ksw2amd_ll_sub_batch_flat.
 * The shoulder of the best hit.  Below the best cell the best column carries H(te + k, qe) = score - gapcost(k), and R(te + k) is at least
 * that.  Under a second piece with a small gape2 this decays by gape2 per row, so whenever gape2 < smax the default window
 * ceil(score / smax) ends before the shoulder does and score2 is then the shoulder's first row outside the window, not a second hit.
 * Example: +100 / -100 matrix, costs (4, 2, 24, 1), a 200-residue query matched with one 60-residue gap (score 19916, te 559) gives
 * d = 200 and score2 = 19916 - (24 + 201) = 19691 at te2 = 760, the first row behind the window and a row of unrelated residues.  A
 * caller who wants independent hits only passes an excl sized to (score - gapo2) / gape2.  The default is kept as it is: it is what
 * makes these entries equal the single-piece ones under equal pieces. */
int ksw2amd_lld_sub_batch(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int excl, int n,
                          const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res, ksw2amd_lsub_t *sub);
int ksw2amd_lld_sub_batch_flat(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int excl, int n,
                               const ksw2amd_lflat_t *in, ksw2amd_lres_t *res, ksw2amd_lsub_t *sub);
/* one pair on a ksw_ll_qinit profile; each returns the score.  They are ksw_ll_i16, ksw2amd_ll_align and ksw2amd_ll_sub under the two-piece
 * cost, results equal to row 0 of the batch entries on that pair.  On a device failure or a bad argument they return 0 with the
 * coordinates at -1, n_cigar = 0 and *sub = (0, -1, -1), and report like ksw_ll_i16 (ksw2amd_error_count, ksw2amd_last_error, the
 * handler, KSW2AMD_ABORT_ON_ERROR).  ksw2amd_lld_align on a profile with m = 1 fails that way, as ksw2amd_lld_align_batch rejects m = 1 */
int ksw2amd_lld(void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int *qe, int *te);
int ksw2amd_lld_align(void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int flag, ksw2amd_laln_t *aln);
int ksw2amd_lld_sub(void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int excl,
                    int *qe, int *te, ksw2amd_lsub_t *sub);

/* Semi-global alignment (new): the whole query, end to end, against the best-scoring interval of
 * the target -- what other libraries call fit, glocal or infix alignment.  Scoring arguments as for ksw2amd_ll_batch: s(t, q) =
 * mat[t * m + q], a gap of length l costs gapo + l * gape, m 1..127, gapo / gape 0..127, every residue code < m.  With t the target index
 * and j the query index, both 0-based, and -1 the boundary:
 *   H(t, -1) = 0 for every t >= -1 (the start in the target is free),   H(-1, j) = -(gapo + (j + 1) * gape),
 *   H(t, j)  = max(H(t - 1, j - 1) + s(t, j), E(t, j), F(t, j)), Gotoh E / F as in ksw_extz (a gap may follow a gap of the other kind at
 *              the cost of another open; E and F are -infinity on the boundary); there is NO clamp at 0;
 *   score = max over 0 <= t < tlen of H(t, qlen - 1),   te = the smallest such t,   qe = qlen - 1.
 * Scores may be negative, and the interval may be empty: when inserting the whole query is best, score = -(gapo + qlen * gape), te = 0.
 * Nothing is launched for qlen <= 0 -> (0, -1, -1), nor for tlen <= 0 with qlen > 0 -> (-(gapo + qlen * gape), qlen - 1, -1).
 * Exact int32; a pair with gapo + qlen * (gape + smax) + smax > 0x3fffffff, smax = max(0, largest matrix entry), is rejected.  A matrix
 * without a positive entry is legal here (the local entries skip such pairs; these do not).  Every argument and every code is checked
 * before anything is staged or launched (KSW2AMD_E_PARAM); the flat entry checks the codes on the device, chunk by chunk, and has the
 * chunking, reset and error semantics and the on_device behaviour of ksw2amd_ll_batch_flat.
 * Free query ends (overlap alignment): ksw2amd_ov_batch further below.  Not computed: a suboptimal score (the start tb and a CIGAR:
 * ksw2amd_sg_align_batch below; the two-piece gap cost: ksw2amd_sgd_batch further below).
 * ksw2amd_sg: one pair on a ksw_ll_qinit profile; returns the score, equal to row 0 of ksw2amd_sg_batch on that pair.  On a device
 * failure or a bad argument it returns 0 with *qe = *te = -1 and reports like ksw_ll_i16 (ksw2amd_error_count, ksw2amd_last_error, the
 * handler, KSW2AMD_ABORT_ON_ERROR). */
int ksw2amd_sg_batch(int m, const int8_t *mat, int gapo, int gape, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res);
int ksw2amd_sg_batch_flat(int m, const int8_t *mat, int gapo, int gape, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res);
int ksw2amd_sg(void *q, int tlen, const uint8_t *target, int gapo, int gape, int *qe, int *te);

/* Semi-global alignment with the interval's start and a CIGAR (new): what a read mapper needs
 * after ksw2amd_sg_batch -- target[tb..te] and the path -- as one call instead of a host reversal and two more batch calls.  For every pair:
 *   score, qe, te   bit for bit what ksw2amd_sg_batch returns; qb = 0 whenever qlen > 0;
 *   tb              with G(x) the global score of the whole query against target[x..te] under the scalar ksw_extz contract (w = -1,
 *                   zdrop = -1), and G(te + 1) = -(gapo + qlen * gape), the empty interval with the whole query inserted: the LARGEST x
 *                   in [0, te + 1] with G(x) == score -- the shortest optimal interval (such an x always exists).  tb == te + 1 says that
 *                   the interval is empty; it is the answer whenever inserting the whole query is optimal (the empty interval wins its
 *                   ties), where ksw2amd_sg_batch reports te = 0, so tb = 1.  In the reference's terms: with r = ksw_extz(reverse(query),
 *                   reverse(target[0..te]), w = -1, zdrop = -1, KSW_EZ_SCORE_ONLY), tb = te - r.mqe_t when r.mqe > -(gapo + qlen * gape),
 *                   te + 1 otherwise;
 *   cigar           non-empty interval: exactly the CIGAR of the scalar ksw_extz(km, qlen, query, te-tb+1, target+tb, m, mat, gapo, gape,
 *                   -1, -1, KSW_EZ_GENERIC_SC | (flag & (KSW_EZ_RIGHT | KSW_EZ_REV_CIGAR)), &ez), whose score equals `score` (checked for
 *                   every pair; a mismatch is reported as an error, never returned).  Empty interval: the one operation qlen I
 *                   (qlen << 4 | 1).
 * flag: KSW_EZ_SCORE_ONLY (coordinates only, n_cigar = 0, no third stage), KSW_EZ_RIGHT, KSW_EZ_REV_CIGAR; any other bit is
 * KSW2AMD_E_PARAM.  Nothing is launched for qlen <= 0 -> score 0, qb = qe = tb = te = -1, n_cigar 0; nor for tlen <= 0 with qlen > 0 ->
 * score -(gapo + qlen * gape), qb 0, qe qlen - 1, te -1, tb 0, and the CIGAR qlen I unless KSW_EZ_SCORE_ONLY.  Arguments, ranges (the
 * 0x3fffffff limit included) and residue codes as for ksw2amd_sg_batch, all checked before anything is staged or launched; a matrix
 * without a positive entry is legal; aln == NULL with n > 0 is KSW2AMD_E_PARAM.  The start pass runs on the device from what the forward
 * pass left there (no download, host reversal or second upload in between).  aln[] is zero-initialised by the caller or holds reusable
 * CIGAR buffers (cigar / m_cigar, grown through km), as for ksw2amd_ll_align_batch.  The flat entry has the chunking, the on-device code
 * check, the reset and error semantics and the on_device behaviour of ksw2amd_ll_align_batch_flat (device arena: the spans of the aligned
 * intervals come back once for the CIGAR stage; on a failure every aln[] entry holds score 0, coordinates -1, n_cigar 0).
 * ksw2amd_sg_align: one pair on a ksw_ll_qinit profile; returns the score; on a failure 0 with those reset values, reported like
 * ksw_ll_i16.  Device failures: a negative code, no CPU fallback.
 * Free query ends: ksw2amd_ov_batch and ksw2amd_ov_align_batch further below.  Not computed: a suboptimal score (the two-piece gap cost:
 * ksw2amd_sgd_align_batch below). */
int ksw2amd_sg_align_batch(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n,
                           const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln);
int ksw2amd_sg_align_batch_flat(void *km, int m, const int8_t *mat, int gapo, int gape, int flag, int n,
                                const ksw2amd_lflat_t *in, ksw2amd_laln_t *aln);
int ksw2amd_sg_align(void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int flag, ksw2amd_laln_t *aln);

/* Semi-global alignment under the two-piece gap cost of ksw_extd (new): the six entries above with
 * (gapo2, gape2) after gape, as in the ksw2amd_lld_* entries.  A gap of length l >= 1 costs
 *   cost(l) = min(gapo + l * gape, gapo2 + l * gape2),
 * the cost of the reference's scalar ksw_extd, which never swaps or orders the two pieces; neither do these entries.
 * Score and te: H(t, -1) = 0 for every t >= -1, H(-1, j) = -cost(j + 1), H = max(diag + s, E, F, E2, F2) with the four Gotoh states of
 *   ksw_extd, -infinity on the boundary, NO clamp at 0; score = max over t of H(t, qlen - 1), te the smallest such t, qe = qlen - 1.
 *   Nothing is launched for qlen <= 0 -> (0, -1, -1), nor for tlen <= 0 with qlen > 0 -> (-cost(qlen), qlen - 1, -1).
 * Range: the four costs 0..127; m 1..127 for the score entries, 2..127 for ksw2amd_sgd_align_batch / _flat and ksw2amd_sgd_align (the CIGAR
 *   stage is the scalar ksw_extd, which aligns nothing with m = 1: KSW2AMD_E_PARAM, as for ksw2amd_lld_align_batch); every residue code < m;
 *   a pair with cost(qlen) + (qlen + 1) * smax > 0x3fffffff, smax = max(0, largest matrix entry), is KSW2AMD_E_PARAM.
 * tb, qb and the CIGAR (the align entries): as for ksw2amd_sg_align_batch with G(x) taken under the scalar ksw_extd (w = -1, zdrop = -1) and
 *   G(te + 1) = -cost(qlen): tb is the LARGEST x in [0, te + 1] with G(x) == score, the empty interval (tb = te + 1) wins its ties, qb = 0.
 *   In the reference's terms: with r = ksw_extd(reverse(query), reverse(target[0..te]), w = -1, zdrop = -1, KSW_EZ_SCORE_ONLY),
 *   (score, te) is the best max(r.mqe, -cost(qlen)) at the smallest te, and tb = te - r.mqe_t when r.mqe > -cost(qlen), te + 1 otherwise.
 *   The CIGAR of a non-empty interval is exactly that of the scalar ksw_extd(km, qlen, query, te-tb+1, target+tb, m, mat, gapo, gape, gapo2,
 *   gape2, -1, -1, KSW_EZ_GENERIC_SC | (flag & (KSW_EZ_RIGHT | KSW_EZ_REV_CIGAR)), &ez), whose score equals `score` (checked for every
 *   pair; a mismatch is reported as an error, never returned); of an empty interval, qlen I.  flag: KSW_EZ_SCORE_ONLY, KSW_EZ_RIGHT,
 *   KSW_EZ_REV_CIGAR; any other bit is KSW2AMD_E_PARAM.  tlen <= 0 with qlen > 0: score -cost(qlen), qb 0, qe qlen - 1, te -1, tb 0, and the
 *   CIGAR qlen I unless KSW_EZ_SCORE_ONLY.
 * Equal pieces: with (gapo2, gape2) = (gapo, gape), or with gapo2 >= gapo and gape2 >= gape, every field of every result equals the
 *   corresponding ksw2amd_sg_* entry's.
 * Everything else is as for the ksw2amd_sg_* entries: every argument checked before anything is staged or launched, flat chunking, the
 * on-device code check, the reset values on a failure, on_device arenas, no CPU fallback, KSW2AMD_LL_FORM / KSW2AMD_LL_LDS /
 * KSW2AMD_LL_CHUNK_BYTES; the single-pair entries report failures like ksw_ll_i16.
 * Free query ends: ksw2amd_ovd_batch below.  Not computed: a suboptimal score. */
int ksw2amd_sgd_batch(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res);
int ksw2amd_sgd_batch_flat(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int n, const ksw2amd_lflat_t *in, ksw2amd_lres_t *res);
int ksw2amd_sgd(void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int *qe, int *te);
int ksw2amd_sgd_align_batch(void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int flag, int n, const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln);
int ksw2amd_sgd_align_batch_flat(void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int flag, int n, const ksw2amd_lflat_t *in, ksw2amd_laln_t *aln);
int ksw2amd_sgd_align(void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int flag, ksw2amd_laln_t *aln);

/* Overlap alignment (new): ksw2amd_sg_batch / ksw2amd_sgd_batch with the query's ends free as `ends`
 * says.  Both bits: overlap (dovetail) alignment, the suffix of one sequence against the prefix of the other, or one contained in the
 * other; one bit: the query may hang over the left (QBEG) or the right (QEND) end of the target, as adapter trimming and clipping at a
 * contig edge need.  The target's two ends are always free.  cost(l) = gapo + l * gape for the ov entries, min(gapo + l * gape, gapo2 + l * gape2)
 * with the pieces as the caller orders them for the ovd entries; t the target index, j the query index, -1 the boundary:
 *   H(t, -1) = 0 for every t >= -1;   H(-1, j) = 0 if ends & KSW2AMD_OV_QBEG, else -cost(j + 1);   the gap states are -infinity on the boundary;
 *   the recurrence is that of ksw_extz / ksw_extd, with NO clamp at 0;
 *   candidates: the cells (t, qlen - 1), 0 <= t < tlen, and with ends & KSW2AMD_OV_QEND the cells (tlen - 1, j), 0 <= j < qlen, as well -- real
 *   cells only, never the boundary row or column, so the score may be slightly negative even with both bits;
 *   result: the largest H over the candidates, then the smallest te, then the smallest qe (a tie between the last column and the last row goes
 *   to the last column, ties inside the last row to the smaller column).
 * ends: any other bit is KSW2AMD_E_PARAM, checked before anything is staged; ends == 0 returns ksw2amd_sg_batch's (ksw2amd_sgd_batch's) result
 * bit for bit.  Nothing is launched for qlen <= 0 -> (0, -1, -1), nor for tlen <= 0 with qlen > 0 -> ((ends & KSW2AMD_OV_QBEG) ? 0 :
 * -cost(qlen), qlen - 1, -1), whatever KSW2AMD_OV_QEND says.
 * In the reference's terms: with r = ksw_extz(reverse(query[0..qe]), reverse(target[0..te]), w = -1, zdrop = -1, KSW_EZ_SCORE_ONLY) (ksw_extd
 * for the ovd entries), the value of a cell (te, qe) is max(r.mqe, -cost(qe + 1)), and with KSW2AMD_OV_QBEG max(r.mqe, -cost(qe + 1), r.mte,
 * -cost(te + 1)); the result is the best value over the candidates under the tie rule.
 * Equal pieces: with (gapo2, gape2) = (gapo, gape), or with gapo2 >= gapo and gape2 >= gape, the ovd entries equal the ov entries in every field.
 * Scoring arguments, ranges, residue codes, the 0x3fffffff rejection, flat chunking, the on-device code check, the reset values, on_device
 * arenas and error reporting are exactly those of ksw2amd_sg_batch / ksw2amd_sgd_batch; no CPU fallback.  ksw2amd_ov / ksw2amd_ovd: one pair on
 * a ksw_ll_qinit profile, failures reported like ksw_ll_i16.
 * The start cell and a CIGAR of this mode: ksw2amd_ov_align_batch below.  Not computed: a suboptimal score. */
#define KSW2AMD_OV_QBEG 1   /* the query's start is free: a query prefix may stay unaligned at no cost */
#define KSW2AMD_OV_QEND 2   /* the query's end is free:   a query suffix may stay unaligned at no cost */
int ksw2amd_ov_batch      (int m, const int8_t *mat, int gapo, int gape, int ends, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res);
int ksw2amd_ov_batch_flat (int m, const int8_t *mat, int gapo, int gape, int ends, int n, const ksw2amd_lflat_t *in,    ksw2amd_lres_t *res);
int ksw2amd_ov            (void *q, int tlen, const uint8_t *target, int gapo, int gape, int ends, int *qe, int *te);
int ksw2amd_ovd_batch     (int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int ends, int n, const ksw2amd_lpair_t *pairs, ksw2amd_lres_t *res);
int ksw2amd_ovd_batch_flat(int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int ends, int n, const ksw2amd_lflat_t *in,    ksw2amd_lres_t *res);
int ksw2amd_ovd           (void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int ends, int *qe, int *te);

/* Overlap alignment with the start cell and a CIGAR (new): the ov / ovd entries above as one call in
 * the three stages of ksw2amd_sg_align_batch -- the forward pass, the anchored start pass on the device from what the forward pass left there,
 * the CIGAR stage.  The argument lists are those of the sg_align / sgd_align entries with `ends` placed as in ksw2amd_ov_batch.
 * score, qe, te: bit for bit what ksw2amd_ov_batch / ksw2amd_ovd_batch return for the same `ends`.
 * tb, qb: let G(tb, qb) be the global score of query[qb..qe] against target[tb..te] under the scalar ksw_extz (ksw_extd for the ovd entries)
 *   with w = -1, zdrop = -1; G = -cost(qe - qb + 1) when the target interval is empty (tb = te + 1), -cost(te - tb + 1) when the query interval
 *   is empty (qb = qe + 1).  The candidate start cells are (tb, 0), 0 <= tb <= te + 1, and with ends & KSW2AMD_OV_QBEG also (0, qb),
 *   0 <= qb <= qe + 1.  score equals the largest G over the candidates (the identity stated above in the reference's terms), and (tb, qb) is
 *   the candidate with G == score that has the LARGEST tb, then the LARGEST qb -- the tie rule of ksw2amd_ll_align_batch.  So: the empty target
 *   interval (te + 1, 0) wins every tie, as in ksw2amd_sg_align_batch; a start inside the target (tb > 0, qb = 0) beats a start in row 0; within
 *   row 0 the shortest query interval wins, the empty one (qb = qe + 1) before all others; the corner (0, 0) loses every tie.
 *   qb is NOT qe - r.mte_q of the reference's reversed call: ksw_extz's left-aligned and score-only loops keep the LARGEST column on ties
 *   (max > h ? max_j : j), these entries the smallest.
 * ends == 0: every field of every result equals ksw2amd_sg_align_batch's (ksw2amd_sgd_align_batch's).
 * Equal pieces: with (gapo2, gape2) = (gapo, gape), or with gapo2 >= gapo and gape2 >= gape, the ovd entries equal the ov entries in every field.
 * CIGAR: both intervals non-empty -- exactly that of the scalar ksw_extz(km, qe-qb+1, query+qb, te-tb+1, target+tb, m, mat, gapo, gape, -1, -1,
 *   KSW_EZ_GENERIC_SC | (flag & (KSW_EZ_RIGHT | KSW_EZ_REV_CIGAR)), &ez) (ksw_extd with gapo2, gape2 for ovd), whose score equals `score`
 *   (checked for every pair; a mismatch is reported as an error, never returned); empty target interval: the one operation (qe + 1) I; empty
 *   query interval: the one operation (te + 1) D.
 * flag: KSW_EZ_SCORE_ONLY (coordinates only, n_cigar = 0, no third stage), KSW_EZ_RIGHT, KSW_EZ_REV_CIGAR; any other bit, and any other bit of
 *   ends, is KSW2AMD_E_PARAM, checked before anything is staged.
 * Nothing is launched for qlen <= 0 -> score 0, the four coordinates -1, n_cigar 0; nor for tlen <= 0 with qlen > 0: without KSW2AMD_OV_QBEG
 *   score -cost(qlen), qb 0, qe qlen - 1, te -1, tb 0, CIGAR qlen I (unless KSW_EZ_SCORE_ONLY); with it score 0, qb qlen, qe qlen - 1, te -1,
 *   tb 0, n_cigar 0 -- the whole query hangs over the target.
 * Range: as for ksw2amd_ov_batch / ksw2amd_ovd_batch, the 0x3fffffff rejection included; the ovd align entries take m 2..127 (the scalar
 *   ksw_extd aligns nothing with m = 1), as ksw2amd_sgd_align_batch does.  aln == NULL with n > 0 is KSW2AMD_E_PARAM.
 * The flat entries have the chunking, the on-device code check, the reset of every aln[] entry on a failure and the on_device behaviour of
 * ksw2amd_sg_align_batch_flat (device arena: the span of [qoff + qb, qoff + qe] and [toff + tb, toff + te] comes back once for the CIGAR
 * stage); the single-pair entries report failures like ksw_ll_i16.  No CPU fallback.  Not computed: a suboptimal score. */
int ksw2amd_ov_align_batch      (void *km, int m, const int8_t *mat, int gapo, int gape, int ends, int flag, int n, const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln);
int ksw2amd_ov_align_batch_flat (void *km, int m, const int8_t *mat, int gapo, int gape, int ends, int flag, int n, const ksw2amd_lflat_t *in,    ksw2amd_laln_t *aln);
int ksw2amd_ov_align            (void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int ends, int flag, ksw2amd_laln_t *aln);
int ksw2amd_ovd_align_batch     (void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int ends, int flag, int n, const ksw2amd_lpair_t *pairs, ksw2amd_laln_t *aln);
int ksw2amd_ovd_align_batch_flat(void *km, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int ends, int flag, int n, const ksw2amd_lflat_t *in,    ksw2amd_laln_t *aln);
int ksw2amd_ovd_align           (void *km, void *q, int tlen, const uint8_t *target, int gapo, int gape, int gapo2, int gape2, int ends, int flag, ksw2amd_laln_t *aln);

/* The same in three phases, for callers that keep batches resident in HBM (and for benchmarking the
 * device part alone): create = pack + upload, run = kernels only (asynchronous on `stream`, a hipStream_t
 * or NULL), fetch = wait + download + fill ez[]. */
typedef struct ksw2amd_plan_s ksw2amd_plan_t;
ksw2amd_plan_t *ksw2amd_plan_create(int dual, const ksw2amd_scoring_t *sc, int n, const ksw2amd_pair_t *pairs);
int  ksw2amd_plan_run(ksw2amd_plan_t *plan, void *stream);
int  ksw2amd_plan_fetch(ksw2amd_plan_t *plan, void *km, ksw_extz_t *ez);
void ksw2amd_plan_destroy(ksw2amd_plan_t *plan);
/* a resident plan from a flat batch (host or device arena); run / fetch / timing / cells / destroy as below.  The upload is complete
 * when this returns, but the plan BORROWS the arena: its bytes must stay valid and unchanged until ksw2amd_plan_destroy -- a fetch
 * reads the sequences there for =/X CIGARs (KSW_EZ_EQX) and for the pairs it runs again (wildcard codes met by a packed kernel,
 * alignments the deferred arg-max kernels handed back).  The batch entry points above borrow the arena for the duration of the call only. */
ksw2amd_plan_t *ksw2amd_plan_create_flat(int dual, const ksw2amd_scoring_t *sc, int n, const ksw2amd_flat_t *in);
/* device time of the last ksw2amd_plan_run (HIP events on its stream), fill kernels only / fill + traceback; ms */
int  ksw2amd_plan_timing(ksw2amd_plan_t *plan, float *fill_ms, float *total_ms);
/* in-band DP cells of the plan (exact band, all rows counted even if Z-drop stops early) and device bytes held */
int64_t ksw2amd_plan_cells(const ksw2amd_plan_t *plan);
int64_t ksw2amd_plan_device_bytes(const ksw2amd_plan_t *plan);
/* alignments routed to the packed-int16 kernels (two same-shape alignments per lane group) */
int64_t ksw2amd_plan_packed_pairs(const ksw2amd_plan_t *plan);
/* diagnostics: one text line per kernel class the plan's next run launches --
 *   "kernel=pk G=64 C=16 gaps=1 mode=score rebased=1 nomax=0 generic=0 form=ldscodes tasks=1536"
 * (kernel: int32 / mp / pk / pkmp / solo; form: registers / ldsrows / ldscodes / defer, the launch-time choice);
 * ksw_extf2_sse plans: "kernel=extf-lane form=ldsring ring=36 tasks=65536" (extf-lds / extf-hbm / extf-win4 / extf-win8 / extf-lane;
 * form of the lane class: hbm / ldsring with its rows).  Returns the number of lines; extz / extd / extf plans.  Tests use it to
 * assert which kernel an unforced launch took. */
int ksw2amd_plan_describe(const ksw2amd_plan_t *plan, char *buf, int cap);
/* The KSW2AMD_* environment switches (tuning, A/B runs, tests) are read once per process; this reads them again. */
void ksw2amd_reload_env(void);
/* pairs that a fetch ran a second time through the ordinary kernels since the library was loaded: flat batches' wildcard pairs, and
 * alignments in which the deferred arg-max kernels could not rule out a Z-drop without the arg-max columns */
int64_t ksw2amd_rerun_count(void);
/* Streamed plans (new; replaces nothing in the reference): a one-shape score-only batch handed to the batch entry points runs as ONE
 * plan whose sequence arena goes up in pieces while a single launch per kernel class runs under the upload, each wavefront starting its
 * task when the task's pieces have landed.  out[0] = streamed plans run since the library was loaded, out[1] = runs in which a
 * launch gave up waiting for its inputs (bounded wait) and the plan was run again behind its upload.  KSW2AMD_STREAM=0 / 1:
 * never / every plan that can. */
void ksw2amd_stream_stats(int64_t out[2]);
/* a resident plan of SSE-compatible alignments (every pair, whatever its flags); run / fetch / timing / cells / destroy as above */
ksw2amd_plan_t *ksw2amd_sse_plan_create(int dual, const ksw2amd_scoring_t *sc, int n, const ksw2amd_pair_t *pairs);
/* a resident plan of splice-aware extensions; run / fetch / timing / cells / destroy as above */
ksw2amd_plan_t *ksw2amd_exts_plan_create(const ksw2amd_splice_t *sc, int n, const ksw2amd_spair_t *pairs);
/* a resident plan of gap-linear X-drop extensions; run / fetch / timing / cells / destroy as above */
ksw2amd_plan_t *ksw2amd_extf_plan_create(int8_t mch, int8_t mis, int8_t e, int n, const ksw2amd_fpair_t *pairs);
/* raw device results without the host-side ez[] assembly: 16 int32 per pair
 * {max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end, n_cigar, rows_done, ti, tj, 0, 0} */
int  ksw2amd_plan_fetch_raw(ksw2amd_plan_t *plan, int32_t *out16);
/* diagnostics: the plan's output buffers back to what a freshly created plan may hold -- result records zeroed, traceback and CIGAR
 * scratch filled with 0xA5 bytes; sequences, pair records, task lists and the boundary scratch stay.  A run after it has to produce
 * every record again (tests of repeated runs).  Works on the plan's last stream and synchronises it. */
int  ksw2amd_plan_scrub(ksw2amd_plan_t *plan);

#ifdef __cplusplus
}
#endif
#endif
