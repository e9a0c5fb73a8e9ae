/*
 * bpsw.h -- C ABI of libbPSW_hip.so, the MI355X (gfx950) batched Smith-Waterman plug-in for
 * CS-BWAMEM (ytchen0323/cloud-scale-bwamem).
 *
 * The library is a drop-in for the reference's two native plug-in points; the JNI symbols the
 * Scala driver binds are exported by the same .so (csrc/bpsw_jni.cpp) and are thin marshalling
 * shims over the functions declared here:
 *
 *   boundary 2  SWExtendFPGAJNI.swExtendFPGAJNI(n, bytes)          -> bpsw_extend_batch
 *               replaces src/main/jni_fpga/sw_extend_fpga.c:116-193 + src/main/alphadata/shm_host.c
 *               (declared at src/main/scala/cs/ucla/edu/bwaspark/jni/SWExtendFPGAJNI.scala:22,
 *                called at  .../worker1/MemChainToAlignBatched.scala:175-176)
 *   boundary 1  MateSWJNI.mateSWJNI(opt,pacLen,pes,n,seqs,regs,refs,refSizes) -> bpsw_matesw_group
 *               replaces src/main/native/jni_mate_sw.c:58-662 + native/bwamem_pair.c:115-228
 *               (declared at .../jni/MateSWJNI.scala:24-25, called at .../worker2/MemSamPe.scala:2091-2092)
 *
 * All pointers are plain host (or, for the *_device entry points, device) pointers with explicit
 * sizes; no C++/torch types cross this boundary.  Every function returns BPSW_OK (0) or a negative
 * error code; bpsw_last_error() gives the text.  There is NO CPU fallback: if no HIP device is
 * usable the calls fail with BPSW_ERR_DEVICE.
 *
 * Thread safety: a bpsw_ctx_t serialises its own calls with an internal mutex; use one context
 * per host thread (the JNI shim keeps one per thread per device) for concurrency.
 */
#ifndef BPSW_H
#define BPSW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BPSW_OK 0
#define BPSW_ERR_ARG (-1)      /* malformed argument / wire batch */
#define BPSW_ERR_DEVICE (-2)   /* HIP runtime failure or no gfx950 device */
#define BPSW_ERR_CAPACITY (-3) /* caller's output buffer too small */
#define BPSW_ERR_LIMIT (-4)    /* sequence longer than the kernels support */

#define BPSW_ZDROP_SCALA 0 /* SWUtil.scala:194-199 (default: bit-exact vs the Scala extension()) */
#define BPSW_ZDROP_BWA 1   /* native/ksw.c:455-461 */

#define BPSW_RESCUE_C 0     /* bookkeeping of native/bwamem_pair.c + bwamem.c (what -bPSWJNI 1 does today) */
#define BPSW_RESCUE_SCALA 1 /* bookkeeping of MemSamPe.scala:1111-1238 (what -bPSWJNI 0 does) */

#define BPSW_KSW_XBYTE 0x10000
#define BPSW_KSW_XSTOP 0x20000
#define BPSW_KSW_XSUBO 0x40000
#define BPSW_KSW_XSTART 0x80000

/* kernel limits (checked on the host before every launch) */
#define BPSW_EXT_MAX_QLEN 1023  /* per-side query length of an extension task */
#define BPSW_EXT_MAX_RLEN 4095  /* per-side reference length of an extension task */
#define BPSW_SW_MAX_QLEN 512    /* mate length of a rescue job */
#define BPSW_SW_MAX_TLEN 65535  /* window length of a rescue job */

typedef struct bpsw_ctx bpsw_ctx_t;

/* ---- life cycle ------------------------------------------------------------------------- */
int bpsw_device_count(void);
/* device < 0: pick from BPSW_DEVICES / round robin (INTEGRATION.md "device selection").
 * Side effects on the PROCESS, both documented in INTEGRATION.md: the first bpsw_create on a device asks the HIP runtime for
 * interrupt-driven waits on it (hipSetDeviceFlags(hipDeviceScheduleBlockingSync); BPSW_SPIN_WAIT=1 leaves the runtime's default),
 * and the device phases of all contexts of a device share a pool of min(BPSW_STREAM_POOL = 20, GPU_MAX_HW_QUEUES) streams --
 * GPU_MAX_HW_QUEUES must be in the executor's environment before the runtime initialises (unset: 4 queues, one warning on stderr). */
int bpsw_create(int device, bpsw_ctx_t **out);
void bpsw_destroy(bpsw_ctx_t *ctx);
int bpsw_device_of(const bpsw_ctx_t *ctx);
int bpsw_device_cus(const bpsw_ctx_t *ctx); /* compute units of its device: what the kernels' resident-wave counts are sized by */
/* Spark partition -> device (the north_star's "Spark-partition -> device index"; reference: one accelerator per executor,
 * src/main/jni_fpga/sw_extend_fpga.c:116-193).  The devices contexts are spread over are the entries of BPSW_DEVICES
 * ("0,2,3"; an index may repeat; default: every visible device in order); partition p runs on entry p mod count. */
int bpsw_device_slots(void);                  /* number of entries; 0 = no usable device */
int bpsw_device_for_partition(int partition); /* HIP device index of that entry, -1 = no usable device / negative partition */
const char *bpsw_last_error(void); /* thread-local text of the last failing call */
const char *bpsw_version(void); /* "bPSW-hip <major.minor> (gfx950)": structs of this header only ever grow at their end, and the minor
                                   number changes when one does (0.4: bpsw_stats_t::ext_full_relaunches, bpsw_tail_opt_t::rg_id; 0.5: bpsw_stats_t::sw_ring_calls, ext_ring_calls;
                                   0.6: no struct grew -- the FM-index, seeding and worker1 entries below are new) */

/* ---- scoring that boundary 2 does not transmit (zdrop, mat) ------------------ */
/* defaults: MemOptType (datatype/MemOptType.scala:28-73): a=1 b=4 N=-1, zdrop=100, Scala z-drop parse */
int bpsw_set_ext_scoring(bpsw_ctx_t *ctx, const int8_t mat[25], int zdrop, int zdrop_mode);

/* Which of the kernel's EXACT shortcuts may replace the DP of an extension flank (results are identical either
 * way, this is an A/B and test switch): bit 0 closed form for near-exact flanks, bit 1 single-gap certificate, bit 2 its
 * two-gap-open extension, bit 3 one-base gap at the start of a flank, bit 4 tail-row bound, bit 5 evaluate those forms in the
 * one-task-per-lane sift kernel in front of the extension kernel (where, not which).  mask < 0 or 63: all (default).
 * Applies to bpsw_extend_batch* and bpsw_chain2aln_batch on this context. */
int bpsw_set_ext_shortcuts(bpsw_ctx_t *ctx, int mask);

/* ---- boundary 2: batched seed extension -------------------------------------------------- */
/*
 * wire = header(32 B) | task table (32 B x n) | nibble-packed sequences, exactly the byte[] built
 * by runOnFPGAJNI (MemChainToAlignBatched.scala:76-172).  out receives 10 int16 per task
 * (MemChainToAlignBatched.scala:181-188): idx lo, idx hi, qBeg, qEnd, rBeg, rEnd, score,
 * trueScore, width, 0.  out_len is the capacity of out in int16 units (>= 10*n).
 */
int bpsw_extend_batch(bpsw_ctx_t *ctx, const uint8_t *wire, size_t wire_bytes, int16_t *out, size_t out_len);

/* Single-touch form of bpsw_extend_batch for callers that can fill a buffer themselves (the JNI shim: GetByteArrayRegion of
 * swExtendFPGAJNI's byte[] straight into pinned memory, where the reference does one memcpy into its shared-memory segment,
 * src/main/jni_fpga/sw_extend_fpga.c:146-155).  bpsw_extend_stage returns the context's pinned staging block with room for
 * `bytes`; the caller writes the wire batch there and calls bpsw_extend_commit, which runs the batch without copying it again
 * and returns a VIEW of the 10*n int16 results where the kernel wrote them (*out, *out_len int16; valid until the next call on
 * the context; n == 0 gives *out == NULL).  One commit per stage, of at most the `bytes` that were staged (BPSW_ERR_ARG otherwise: the
 * table scan never reads past the pinned block).  One thread per context, as everywhere. */
int bpsw_extend_stage(bpsw_ctx_t *ctx, size_t bytes, uint8_t **buf);
int bpsw_extend_commit(bpsw_ctx_t *ctx, size_t wire_bytes, const int16_t **out, size_t *out_len);

/* Diagnostics: bpsw_extend_batch that also reports, per task and side (side_how[2 t] left, [2 t + 1] right; 2 n bytes), how the
 * result was produced: 0 = the side is empty, 1 = an exact shortcut (bpsw_set_ext_shortcuts), 2 = the DP was swept.  bench.py
 * uses it to split the useful cell updates per second into "DP run" and "closed form". */
int bpsw_extend_batch_classify(bpsw_ctx_t *ctx, const uint8_t *wire, size_t wire_bytes, int16_t *out, size_t out_len, uint8_t *side_how);

/* Same computation with the wire batch and the result already resident in device memory
 * (used by bench.py; d_wire must be 16-byte aligned).  hip_stream is a hipStream_t or NULL for the context's stream.
 * ASYNCHRONOUS: the device-side table scan, the main launch and the scan's read-back are enqueued back to back and the call
 * returns.  The launch is sized for a fixed geometry (sides <= 256 bases) and checks the scan on the device: a malformed batch,
 * or one with longer sides, is left untouched.  The NEXT call on this context, or bpsw_last_kernel_ms, waits for the launch and
 * (a) returns the deferred BPSW_ERR_ARG / BPSW_ERR_LIMIT of a malformed batch, (b) launches a longer-sided batch again with its
 * real geometry.  d_wire / d_out must stay valid until then.  bpsw_swalign2_batch_device behaves the same way, sizing the
 * launch for the geometry of the previous (verified) call on the context; the first call of a context is synchronous. */
int bpsw_extend_batch_device(bpsw_ctx_t *ctx, const void *d_wire, size_t wire_bytes, int n_tasks,
                             void *d_out, void *hip_stream);

/* Host-side mirror of the Scala packer (MemChainToAlignBatched.scala:76-172) for non-JVM callers.
 * SoA task description; sequences are byte-per-base codes 0..4 in `pool` (left_* already reversed). */
typedef struct {
  int32_t n;
  int32_t o_del, e_del, o_ins, e_ins, pen_clip5, pen_clip3, w; /* header fields */
  int32_t mat_max;                                             /* max(mat), feeds the maxIns/maxDel shorts */
  const int32_t *left_qlen, *left_rlen, *right_qlen, *right_rlen;
  const int64_t *left_q_off, *left_r_off, *right_q_off, *right_r_off; /* into pool */
  const int32_t *reg_score, *q_beg, *h0, *idx;
  const uint8_t *pool;
} bpsw_ext_tasks_t;
size_t bpsw_wire_size(const bpsw_ext_tasks_t *t);
int bpsw_wire_pack(const bpsw_ext_tasks_t *t, uint8_t *buf, size_t cap, size_t *bytes);

/* Coordinate batches ("wire format 2"): the same call -- and the same JNI symbol, swExtendFPGAJNI(n, bytes) --
 * accepts a batch that names the target flanks by reference coordinates instead of shipping their bases, when the reference
 * is on the device (bpsw_ref_load).  It replaces bnsGetSeq + the leftRs/rightRs copies + their nibble packing
 * (MemChainToAlignBatched.scala:363, 511-517, 534-541, 143-161) on the caller's side and about a third of the bytes per task.
 *   header      as format 1, with byte 7 = BPSW_WIRE_COORDS (format 1 leaves it 0)
 *   task record 40 bytes: the 32 bytes of format 1 (leftQlen, leftRlen, rightQlen, rightRlen int16; word offset of the task's
 *               nibbles; regScore, qBeg, h0 int16; maxIns/maxDel shorts; idx int32) with the seed length (int16) in the slot of
 *               the redundant 16-bit idx (bytes 18-19), then the seed's rBeg in [0, 2*l_pac) as int64 (bytes 32-39)
 *   nibbles     leftQs then rightQs only (leftQs reversed, as in format 1)
 * The left target flank is base(rBeg - 1 - i), i < leftRlen; the right one base(rBeg + len + i), i < rightRlen, with base() the
 * doubled-strand lookup of bnsGetSeq (util/BNTSeqUtil.scala:56-73); a flank must not leave [0, 2*l_pac) nor bridge the strands
 * (getMaxSpan, MemChainToAlignBatched.scala:654-677, guarantees both).  Results are identical to format 1 on the same tasks. */
#define BPSW_WIRE_COORDS 2
typedef struct {
  int32_t n;
  int32_t o_del, e_del, o_ins, e_ins, pen_clip5, pen_clip3, w; /* header fields */
  int32_t mat_max;
  const int32_t *left_qlen, *left_rlen, *right_qlen, *right_rlen;
  const int64_t *left_q_off, *right_q_off; /* into pool; left flank already reversed */
  const int32_t *reg_score, *q_beg, *h0, *idx, *seed_len;
  const int64_t *seed_rbeg;
  const uint8_t *pool;
} bpsw_ext_coord_tasks_t;
size_t bpsw_wire_coords_size(const bpsw_ext_coord_tasks_t *t);
int bpsw_wire_coords_pack(const bpsw_ext_coord_tasks_t *t, uint8_t *buf, size_t cap, size_t *bytes);

/* ---- boundary 1: pair-end mate-SW rescue -------------------------------------------------- */
typedef struct { /* == mem_alnreg_t native/bwamem.h:49-61 == MemAlnRegType.scala:26-38 */
  int64_t rb, re;
  int32_t qb, qe, score, truesc, sub, csub, sub_n, w, seedcov, secondary;
  uint64_t hash;
} bpsw_alnreg_t; /* 64 bytes */

typedef struct { /* == mem_pestat_t native/bwamem.h:65-69 == MemPeStat.scala:27-31 */
  int32_t low, high, failed, pad_;
  double avg, std;
} bpsw_pestat_t;

typedef struct { /* the MemOptType fields the rescue reads (native/jni_mate_sw.c:177-221) */
  int32_t a, b, o_del, e_del, o_ins, e_ins, pen_unpaired, pen_clip5, pen_clip3, w, zdrop, T, flag,
      min_seed_len, max_ins, max_matesw;
  float mask_level_redun;
  int8_t mat[25];
  int8_t pad_[3];
} bpsw_opt_t;
void bpsw_opt_default(bpsw_opt_t *opt);

/*
 * Raw local-SW jobs (SWUtil.SWAlign2, SWUtil.scala:583-601), one per (anchor, orientation).
 * Job t aligns query bytes q_pool[q_off[t] .. +q_len[t]) -- reverse-complemented on the fly when
 * q_rev[t] != 0 (MemSamPe.scala:1175-1184) -- against t_pool[t_off[t] .. +t_len[t]).
 * out receives 7 int32 per job: score, tEnd, qEnd, score2, tEnd2, tBeg, qBeg.
 */
typedef struct {
  int32_t n;
  int32_t xtra; /* KSW_X* flags | min score, same for all jobs (MemSamPe.scala:1187-1189) */
  const int32_t *q_len, *t_len;
  const int64_t *q_off, *t_off;
  const uint8_t *q_rev;
  const uint8_t *q_pool, *t_pool;
  size_t q_pool_bytes, t_pool_bytes;
} bpsw_sw_jobs_t;
int bpsw_swalign2_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_sw_jobs_t *jobs, int32_t *out);

/* Device-resident form: every array pointer in `jobs` is a device pointer (pools 16-byte aligned). */
int bpsw_swalign2_batch_device(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_sw_jobs_t *jobs,
                               void *d_out, void *hip_stream);

/*
 * The whole boundary-1 call in flat SoA form (what the JNI shim builds from the object arrays):
 *   seq_len/seq_off[2G]   mate sequences (codes 0..4) in seq_pool, index 2k+i
 *   reg_cnt[2G], regs     existing regions concatenated in (k,i,j) order (MemSamPe.scala:1963-1990)
 *   ref_cnt[2G]           refSizeArray (MemSamPe.scala:1944-1947)
 *   ref_rb/re/len/off[4R] per (k,i,j<ref_cnt) x 4 orientations; window bytes at ref_pool+ref_off
 *   out_cnt[2G], out_regs regions after rescue in (k,i,rank) order; *out_total = sum(out_cnt)
 * Returns BPSW_ERR_CAPACITY (with *out_total set to the needed size) if out_cap is too small.
 */
typedef struct {
  int32_t group_size;
  int64_t l_pac;
  bpsw_pestat_t pes[4];
  const int32_t *seq_len;
  const int64_t *seq_off;
  const uint8_t *seq_pool;
  size_t seq_pool_bytes;
  const int32_t *reg_cnt;
  const bpsw_alnreg_t *regs;
  const int32_t *ref_cnt;
  const int64_t *ref_rb, *ref_re, *ref_len, *ref_off;
  const uint8_t *ref_pool;
  size_t ref_pool_bytes;
} bpsw_rescue_group_t;
int bpsw_matesw_group(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_rescue_group_t *g, int mode,
                      int32_t *out_cnt, bpsw_alnreg_t *out_regs, int64_t out_cap, int64_t *out_total);

/* ---- "next" row: banded global alignment -> score + CIGAR ------------------------------ */
/*
 * SWUtil.SWGlobal (SWUtil.scala:233-397 == ksw_global2, native/ksw.c:501-584), the DP behind bwaGenCigar2
 * (MemRegToADAMSAM.scala:738-891).  It is NOT behind either JNI of the reference (the Scala driver calls it
 * directly), so this is an additional export for callers that want CIGARs from the device.
 * Job t aligns q_pool[q_off[t]..+q_len[t]) to t_pool[t_off[t]..+t_len[t]) globally inside the band w[t]
 * (the caller applies the band rule of MemRegToADAMSAM.scala:794-804 and the strand reversal of :764-781).
 * Every job must have w[t] >= |t_len[t] - q_len[t]|: under a narrower band the last cell lies outside the band, neither the
 * Scala nor ksw_global2 defines an alignment there (both return the score -2^30 and an accidental CIGAR), and the call is
 * refused with BPSW_ERR_ARG.  (bwaGenCigar2 never asks for less than |t_len - q_len| + 3.)
 * Scratch: the call reserves max_t(min(q_len, 2w+1) * t_len) bytes of device memory for every wavefront the launch starts
 * (the jobs rounded up to a multiple of 4, at most the waves resident on the device), so one job at both limits takes
 * 4 x 67 MB, and a batch of thousands of such jobs as many times 67 MB as there are resident waves (about two thousand).
 * out_score[t]; out_ncigar[t] = number of operations; out_cigar[t*max_cigar ..] = len<<4|op (0=M 1=I 2=D).
 * If out_ncigar[t] > max_cigar that job's operations were not written: resubmit it with a larger max_cigar (<= 512); a job of
 * more than 512 operations reports its count and cannot be produced.  Only out_ncigar[t] words of a job's row are written, and
 * none of a job that did not fit: the rest of out_cigar is left as the caller passed it.
 */
#define BPSW_GLOBAL_MAX_QLEN 1023
#define BPSW_GLOBAL_MAX_TLEN 65535
#define BPSW_GLOBAL_MAX_CIGAR 512
typedef struct {
  int32_t n;
  int32_t max_cigar;
  const int32_t *q_len, *t_len, *w;
  const int64_t *q_off, *t_off;
  const uint8_t *q_pool, *t_pool;
  size_t q_pool_bytes, t_pool_bytes;
} bpsw_global_jobs_t;
int bpsw_global_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_global_jobs_t *jobs, int32_t *out_score,
                      int32_t *out_ncigar, uint32_t *out_cigar);

/* ---- "next" row: reference-window extraction on the device ------------------------------ */
/*
 * bnsGetSeq (util/BNTSeqUtil.scala:37-79 == bns_get_seq, native/bntseq.c) with the 2-bit .pac resident in HBM
 * (base k = pac[k>>2] >> ((~k & 3) << 1) & 3; coordinates >= l_pac address the reverse-complement strand).  The
 * reference belongs to the DEVICE of the context it was loaded through and is seen by every context of that device
 * (the JNI shim keeps one context per Spark task thread); loading or unloading must not race with calls in flight on
 * that device.  Once loaded, the callers of bnsGetSeq on the hot path (MemSamPe.scala:1852 for the rescue windows)
 * can send only (rBeg, rEnd) instead of the bytes:
 *   bpsw_sw_jobs_t      with t_pool == NULL : t_off[t] is the window start in the doubled coordinate space,
 *                                             t_len[t] its length; a window may not bridge l_pac.
 *   bpsw_rescue_group_t with ref_pool == NULL: ref_rb/ref_re name the windows (-1,-1 = failed orientation,
 *                                             MemSamPe.scala:1863-1868); ref_len/ref_off are ignored, the length is
 *                                             derived with bnsGetSeq's own rules (clamp to [0, 2*l_pac), 0 when the
 *                                             window bridges the strands) and g->l_pac must equal the loaded length.
 * bpsw_ref_fetch is bnsGetSeq itself (n windows -> bytes), for callers that still want the bases on the host and
 * for the parity tests: out_len[t] = window length after the reference's swap/clamp (0 when bridging); the bases go
 * to out_pool[out_off[t] ..]; returns BPSW_ERR_CAPACITY if a window does not fit before out_pool_bytes.
 */
int bpsw_ref_load(bpsw_ctx_t *ctx, const uint8_t *pac, int64_t l_pac); /* copies (l_pac+3)/4 bytes to the device */
int bpsw_ref_unload(bpsw_ctx_t *ctx);
int64_t bpsw_ref_length(const bpsw_ctx_t *ctx); /* l_pac of the loaded reference, 0 if none */
int bpsw_ref_fetch(bpsw_ctx_t *ctx, int32_t n, const int64_t *beg, const int64_t *end, uint8_t *out_pool,
                   size_t out_pool_bytes, const int64_t *out_off, int64_t *out_len);

/* ---- "next" row: the memChainToAlnBatched round loop on the device ----------------------------- */
/*
 * memChainToAlnBatched (worker1/MemChainToAlignBatched.scala:380-616; per chain == mem_chain2aln, native/bwamem.c:552-672):
 * the caller hands over the reads of a batch with their filtered seed chains and gets back, per read, the regions the
 * Scala leaves in regArrays -- all rounds (testExtension, checkOverlapping, extension with band retries, seed coverage)
 * run on the device, one wavefront per read, with the reference windows read from the 2-bit reference loaded by
 * bpsw_ref_load.  One call per batch replaces one swExtendFPGAJNI call per round plus the Scala-side task packing.
 *   read_len/read_off[n]  : reads (codes 0..4, <= 256 bases) in read_pool
 *   chain_cnt[n]          : chains per read (0 == chainsFilteredArray(i) null)
 *   seed_cnt[sum chains]  : seeds per chain, (read, chain) order
 *   seed_rbeg/qbeg/len[]  : MemSeedType fields in (read, chain, seedsRefArray) order; a chain lies on one strand
 *   out_cnt[n], out_regs  : regions per read in creation order (sub, csub, sub_n, secondary, hash = 0 as in the Scala);
 *                           out_cap must be >= the total number of seeds.  With BPSW_C2A_SORT_DEDUP the lists are
 *                           passed through memSortAndDedup (what bwaMemWorker1Batched returns,
 *                           BWAMemWorker1Batched.scala:128-133), C flavour by default, Scala flavour with
 *                           BPSW_C2A_DEDUP_SCALA.
 * zdrop_mode selects the z-drop parse as in bpsw_set_ext_scoring.  Needs e_del, e_ins >= 1 and 1 <= w <= 254.
 */
#define BPSW_C2A_SORT_DEDUP 1
#define BPSW_C2A_DEDUP_SCALA 2
#define BPSW_W1_CHAIN_DEVICE 4 /* bpsw_worker1_batch only: chain and filter the seeds on the device (bpsw_chain_batch's kernels) */
#define BPSW_W1_SEED_PLAN_DEVICE 8 /* bpsw_worker1_batch only: plan the suffix-array pass on the device (as BPSW_SEED_PLAN_DEVICE) */
#define BPSW_W1_CHAINS_RESIDENT 16 /* bpsw_worker1_batch only: BPSW_W1_CHAIN_DEVICE, and the chains stay on the device for the round loop */
typedef struct {
  int32_t n_reads;
  const int32_t *read_len;
  const int64_t *read_off;
  const uint8_t *read_pool;
  size_t read_pool_bytes;
  const int32_t *chain_cnt;
  const int32_t *seed_cnt;
  const int64_t *seed_rbeg;
  const int32_t *seed_qbeg, *seed_len;
} bpsw_chains_t;
int bpsw_chain2aln_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_chains_t *batch, int zdrop_mode, int flags,
                         int32_t *out_cnt, bpsw_alnreg_t *out_regs, int64_t out_cap, int64_t *out_total);

/* ---- worker1 from reads: FM-index seeding on the device, chaining and chain filtering on the host ---------------------------
 *
 * generateChains + memChainFilter (worker1/MemChain.scala, BWTSMem.scala, MemChainFilter.scala); the pinned behaviour is the C
 * they were transcribed from: bwt_smem1 / bwt_extend / bwt_sa (native/bwt.c:85-95, 261-347), smem_next2, mem_insert_seed,
 * mem_chain, mem_chain_flt (native/bwamem.c:117-379).  DESIGN.md lists where the Scala differs in result.
 *
 * The index is what the aligner's .bwt and .sa files hold and BWTType loads: primary, L2[5] (L2[0] == 0), seq_len == L2[4], the
 * uint32 BWT array in the interleaved form of bwt_occ_intv (native/bwt.h: every 128 bases four 64-bit occurrence counts, then eight
 * words of 2-bit bases; bwt_size == (seq_len + 15) / 16 + ((seq_len + 127) / 128 + 1) * 8 words), sa_intv (a power of two), n_sa ==
 * (seq_len + sa_intv) / sa_intv and the sampled suffix array with sa[0] == -1.  Like the reference of bpsw_ref_load it belongs to
 * the DEVICE of the context it was loaded through, is seen by every context of that device, and must not be loaded or unloaded
 * while calls are in flight on it.  It stays on the device until bpsw_fmi_unload (or the end of the process): bpsw_destroy of the
 * loading context does not free it, as it does not free the reference.  BPSW_ERR_ARG for a bwt_size, sa_intv or n_sa that
 * contradicts seq_len. */
int bpsw_fmi_load(bpsw_ctx_t *ctx, int64_t primary, const int64_t L2[5], int64_t seq_len, const uint32_t *bwt, int64_t bwt_size,
                  int32_t sa_intv, int64_t n_sa, const int64_t *sa);
int bpsw_fmi_unload(bpsw_ctx_t *ctx);
int64_t bpsw_fmi_length(const bpsw_ctx_t *ctx); /* seq_len of the loaded index, 0 if none */

#define BPSW_MEM_F_NO_EXACT 0x40 /* native/bwamem.h:19: what bpsw_seed_opt_t.no_exact stands for */
#define BPSW_SEED_MAX_QLEN 256   /* read length of the seeding entries: the round loop's limit (bpsw_chain2aln_batch) */
typedef struct { /* the mem_opt_t fields seeding, chaining and the chain filter read (native/bwamem.h:21-47) */
  int32_t min_seed_len, max_occ, split_width, max_chain_gap, no_exact;
  float split_factor, chain_drop_ratio, mask_level;
} bpsw_seed_opt_t;
void bpsw_seed_opt_default(bpsw_seed_opt_t *s); /* == mem_opt_init, native/bwamem.c:45-74 */

typedef struct { /* reads: codes 0..4 in read_pool, at most BPSW_SEED_MAX_QLEN bases each */
  int32_t n_reads;
  const int32_t *read_len;
  const int64_t *read_off;
  const uint8_t *read_pool;
  size_t read_pool_bytes;
} bpsw_reads_t;
typedef struct { /* one bi-interval of smem_next2 (bwtintv_t: x[3], info = qbeg << 32 | qend), in the order the reference visits them */
  int64_t x0, x1, x2;
  int32_t qbeg, qend;
  int32_t kept; /* 1: passes mem_insert_seed's filter (qend - qbeg >= min_seed_len and x2 <= max_occ), 0: skipped there */
  int32_t pad_;
} bpsw_smem_t; /* 40 bytes */
typedef struct { /* mem_seed_t, native/bwamem.c:167-170 */
  int64_t rbeg;
  int32_t qbeg, len;
} bpsw_seed_t; /* 16 bytes */

/* The device part alone: per read the bi-intervals of every smem_next2 call until the read is used up (BEFORE the filter; `kept`
 * records its verdict) and the seeds of the kept ones -- bwt_sa(x0 + k), interval order then k ascending, seeds bridging l_pac ==
 * seq_len / 2 dropped (native/bwamem.c:228) -- both lists concatenated in read order.  A read shorter than min_seed_len has no
 * intervals and no seeds (mem_chain returns before seeding).  BPSW_ERR_CAPACITY with *intv_total / *seed_total set to what is
 * needed when a list does not fit; BPSW_ERR_LIMIT for a read longer than BPSW_SEED_MAX_QLEN; BPSW_ERR_ARG when no index is loaded. */
int bpsw_seed_batch(bpsw_ctx_t *ctx, const bpsw_seed_opt_t *sopt, const bpsw_reads_t *reads, int32_t *intv_cnt, bpsw_smem_t *intv,
                    int64_t intv_cap, int64_t *intv_total, int32_t *seed_cnt, bpsw_seed_t *seeds, int64_t seed_cap,
                    int64_t *seed_total);

/* bpsw_seed_batch with flags.  0: bpsw_seed_batch itself.  BPSW_SEED_PLAN_DEVICE: the tables of the suffix-array pass (which
 * intervals are kept, the prefix sums of their x2) are made on the device by two kernels and a device-wide scan, from the interval
 * rows where the search left them, instead of by the calling thread from rows copied to the host; seed_cnt and seeds are what
 * bpsw_seed_batch gives, and intv_cnt and *intv_total are still returned.  intv == NULL (with intv_cap == 0) is allowed: then no
 * interval leaves the device -- per read the counts (4 bytes), the occurrence offsets (8 bytes) and the seeds come back.  A non-null
 * intv gets the intervals as well, fetched for the caller only.  Any other flag is BPSW_ERR_ARG. */
#define BPSW_SEED_PLAN_DEVICE 1
int bpsw_seed_batch_ex(bpsw_ctx_t *ctx, const bpsw_seed_opt_t *sopt, const bpsw_reads_t *reads, int32_t *intv_cnt, bpsw_smem_t *intv,
                       int64_t intv_cap, int64_t *intv_total, int32_t *seed_cnt, bpsw_seed_t *seeds, int64_t seed_cap,
                       int64_t *seed_total, int flags);
/* Diagnostics.  b[0], b[1]: the bytes staged to the device and fetched from it by the calling thread's most recent seeding stage
 * (bpsw_seed_batch, bpsw_seed_batch_ex, or the seeding stage of bpsw_worker1_batch): what was copied, as bpsw_last_worker1_times
 * says what was waited.  bpsw_scan_set_tile: the items one workgroup of the device scan takes (bpsw_scan.hip), process-wide; 0 = the
 * default (2 048), other values are rounded up to a multiple of 64.  The tests lower it to reach several tiles, and a second level
 * that loops, with a few thousand reads. */
void bpsw_last_seed_bytes(int64_t b[2]);
void bpsw_scan_set_tile(int items);

/* Host only (no context, no GPU), one read: its seeds in emission order -> chains.  Chaining is mem_insert_seed's tree side
 * (test_and_merge against the chain with the largest pos <= rbeg, else a new chain; the chains come out in the B-tree's in-order
 * traversal, chains of equal pos included, in the order kbtree.h leaves them); with `filter` != 0 mem_chain_flt follows.
 * w is mem_opt_t.w (bpsw_opt_t.w).  Output in the shape of bpsw_chains_t: chain_seed_cnt[chain] and the seeds concatenated;
 * chain_cap >= n_seeds and out_seeds of n_seeds entries always suffice.  Returns the number of chains or a negative error. */
int bpsw_chain_seeds(const bpsw_seed_opt_t *sopt, int32_t w, int64_t l_pac, int32_t n_seeds, const bpsw_seed_t *seeds, int32_t filter,
                     int32_t *chain_seed_cnt, int32_t chain_cap, bpsw_seed_t *out_seeds);

/* The same for a batch, on the device (chain_kernel, one read per lane): read r's seeds are the next seed_cnt[r] of `seeds`.  Per
 * read the result is exactly bpsw_chain_seeds', concatenated in read order: chain_cnt[read], chain_seed_cnt[chain], out_seeds.
 * BPSW_ERR_CAPACITY with *chain_total / *seed_total set to what is needed when chain_cap or seed_cap is too small (the sum of
 * seed_cnt always suffices for both); BPSW_ERR_ARG for a seed with len < 1 or qbeg < 0; n_reads == 0 and reads without seeds are
 * fine.  Reads of more than BPSW_CHAIN_DEV_MAX_SEEDS seeds (environment, read once; default 128, 0 = no limit) are chained by
 * bpsw_chain_seeds on the calling thread while the kernel runs. */
int bpsw_chain_batch(bpsw_ctx_t *ctx, const bpsw_seed_opt_t *sopt, int32_t w, int64_t l_pac, int32_t n_reads, const int32_t *seed_cnt,
                     const bpsw_seed_t *seeds, int32_t filter, int32_t *chain_cnt, int32_t *chain_seed_cnt, int64_t chain_cap,
                     bpsw_seed_t *out_seeds, int64_t seed_cap, int64_t *chain_total, int64_t *seed_total);
/* Diagnostics.  The byte budget of the chain kernel's workspace arena, process-wide (0 = the default, 256 MB): a batch runs in
 * slices of reads that fit it, a single read larger than the budget grows the arena to that read.  The tests lower it to reach
 * both with small batches.  bpsw_chain_last_split: how the calling thread's most recent chain stage (bpsw_chain_batch, or
 * bpsw_worker1_batch with BPSW_W1_CHAIN_DEVICE) was divided: reads chained by the kernel, reads chained on the calling thread,
 * slices, bytes of arena asked for. */
void bpsw_chain_set_arena_budget(int64_t bytes);
void bpsw_chain_last_split(int64_t st[4]);

/* bpsw_chain_batch with flags.  0: bpsw_chain_batch itself.  BPSW_CHAIN_TABLES_DEVICE: the stage leaves the chains on the device in
 * read order, as the tables the round loop's kernel indexes (what bpsw_worker1_batch does with BPSW_W1_CHAINS_RESIDENT), and the entry
 * then fetches them for the caller only: chain_cnt, chain_seed_cnt and the seeds, zipped back into bpsw_seed_t.  Results, totals and
 * the capacity behaviour are exactly bpsw_chain_batch's.  Any other flag is BPSW_ERR_ARG. */
#define BPSW_CHAIN_TABLES_DEVICE 1
int bpsw_chain_batch_ex(bpsw_ctx_t *ctx, const bpsw_seed_opt_t *sopt, int32_t w, int64_t l_pac, int32_t n_reads, const int32_t *seed_cnt,
                        const bpsw_seed_t *seeds, int32_t filter, int32_t *chain_cnt, int32_t *chain_seed_cnt, int64_t chain_cap,
                        bpsw_seed_t *out_seeds, int64_t seed_cap, int64_t *chain_total, int64_t *seed_total, int flags);
/* Diagnostics.  b[0], b[1]: the bytes staged to the device and fetched from it by the calling thread's most recent chain stage
 * (bpsw_chain_batch, bpsw_chain_batch_ex, or bpsw_worker1_batch with BPSW_W1_CHAIN_DEVICE or BPSW_W1_CHAINS_RESIDENT), in the manner of
 * bpsw_last_seed_bytes; the copy bpsw_chain_batch_ex makes for its caller is not counted.  With the chains resident the stage
 * fetches 32 bytes a slice of the arena (an error word and the slice's totals) and 32 bytes of totals once, whatever the number of
 * reads, plus the seeds of the reads it chains on the calling thread (BPSW_CHAIN_DEV_MAX_SEEDS) when those are on the device only. */
void bpsw_last_chain_bytes(int64_t b[2]);

/* worker1 from reads to regions: bpsw_seed_batch, bpsw_chain_seeds with the filter per read, then bpsw_chain2aln_batch as it is
 * (zdrop_mode, flags, out_* exactly as there; *out_total is set to the needed out_cap on BPSW_ERR_CAPACITY).  Needs the reference
 * (bpsw_ref_load) and an index with seq_len == 2 * l_pac on the context's device.  With BPSW_W1_CHAIN_DEVICE in flags the seeds
 * stay on the device and are chained and filtered there (as bpsw_chain_batch does; seeds bridging l_pac dropped by the kernel), and
 * only the chains come back; the regions are the same.  With BPSW_W1_SEED_PLAN_DEVICE the seeding stage plans its suffix-array pass on
 * the device (bpsw_seed_batch_ex) and the intervals do not come back; with both flags the seeding stage fetches per read its interval
 * count and its occurrence offset and nothing else.  With BPSW_W1_CHAINS_RESIDENT (which implies BPSW_W1_CHAIN_DEVICE and composes
 * with the other flags) the chains do not come back either: the chain stage leaves on the device, in read order, the tables the round
 * loop's kernel indexes, and the round loop runs on them; with all three flags nothing is fetched between the reads going out and the
 * regions coming back except counts and totals.  The seeds are then not validated as bpsw_chain2aln_batch validates a caller's (inside
 * their read, on one strand, inside the reference): the library's own kernels produced them.  out_cnt, the regions and the capacity
 * contract are bit-identical.  None of the three flags is passed on to the round loop. */
int bpsw_worker1_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_reads_t *reads, int zdrop_mode,
                       int flags, int32_t *out_cnt, bpsw_alnreg_t *out_regs, int64_t out_cap, int64_t *out_total);
/* Diagnostics: the number of lanes (reads in flight, a multiple of 64) seed_smem_kernel keeps resident, process-wide; 0 = the default,
 * 256 per compute unit (bpsw_device_cus).  Each resident lane owns four lists of (longest read of the batch + 1) intervals of 32
 * bytes in a per-context arena: 2.2 GB at 256 bases on 256 CUs.  The tests lower it to reach the grid-stride path with a small batch. */
void bpsw_seed_set_resident_lanes(int lanes);
/* wall time of the calling thread's most recent bpsw_worker1_batch (ms): seeding call, chaining (host or device), round loop call */
void bpsw_last_worker1_times(double ms[3]);

/* ---- the FM-index built on the device from the 2-bit reference (bpsw_index.hip) -----------------------------------------------
 *
 * pac and l_pac are what bpsw_ref_load takes: the forward strand, base k = pac[k >> 2] >> ((~k & 3) << 1) & 3.  The text is the
 * doubled sequence, the forward strand followed by its reverse complement (seq_len == 2 * l_pac); the device reads the second half
 * from the forward bytes, the host never makes it.  The result is what bpsw_fmi_load documents and `bwa index` writes -- the
 * sentinel's row removed from the BWT and recorded as primary, L2[0] == 0 and L2[4] == seq_len, the uint32 array in the
 * interleaved form of bwt_occ_intv, n_sa == (seq_len + sa_intv) / sa_intv samples of the suffix array of text + sentinel at rows
 * 0, sa_intv, 2 sa_intv ... with sa[0] == -1 -- and it is unique: every suffix of text + sentinel is distinct.
 *
 * bpsw_fmi_build_shape (host only) fills seq_len, bwt_size, n_sa and sa_intv: what the caller's arrays have to hold.
 * bpsw_fmi_build writes bwt_size words to bwt and n_sa entries to sa and fills *out.  flags: BPSW_FMI_BUILD_LOAD -- the built index
 * also becomes the device's loaded index, as after bpsw_fmi_load, with no second upload; bwt and sa may then be NULL (each on its
 * own), and the index exists on the device only.  BPSW_FMI_BUILD_REF -- the pac also becomes the device's loaded reference, as after
 * bpsw_ref_load.  Both follow those entries' rules: the index and the reference belong to the device, are seen by every context of
 * it, must not be loaded while calls are in flight on it, and outlive bpsw_destroy.
 *
 * BPSW_ERR_ARG: NULL ctx, pac or out, l_pac < 1, sa_intv < 1 or not a power of two, unknown flag bits, bwt or sa NULL without
 * BPSW_FMI_BUILD_LOAD.  BPSW_ERR_CAPACITY: bwt_cap below out->bwt_size or sa_cap below out->n_sa; the sizes are filled in *out and
 * nothing is built.  BPSW_ERR_LIMIT: the working set does not fit the device memory that is free -- it is computed from seq_len
 * before anything is allocated, about 105 bytes a suffix, and bpsw_last_error names the bytes needed and the
 * bytes available -- or seq_len + 1 is above 2^32 (a round's sort key holds a group and a rank in 64 bits).  BPSW_ERR_DEVICE as
 * elsewhere.  A failed call leaves a previously loaded index and reference as they were.
 *
 * Diagnostics (calling thread's most recent bpsw_fmi_build).  times, ms of wall clock: first keys and first sort, doubling rounds,
 * BWT and counts and packing, sampling and copy-out (and the hand-over of LOAD / REF), the whole call.  stats: [0] doubling rounds
 * run after the first sort, [1] suffixes still unresolved after the first sort, [2] the largest unresolved list over the rounds,
 * [3] radix passes in all, [4] suffixes per workgroup in the sort (its tile), [5] peak device bytes, [6] bases in the first key,
 * [7] 0.  bpsw_fmi_build_set_first_key, process-wide: 0 = the default (29, as many as fit the key), else the number of bases in the
 * first sort key (clamped to 1 .. 29); the tests lower it to reach many rounds on small genomes.  bpsw_fmi_build_set_budget,
 * process-wide: 0 = what the device has free, else the call pretends that this many bytes are. */
#define BPSW_FMI_BUILD_LOAD 1
#define BPSW_FMI_BUILD_REF 2
typedef struct {
  int64_t primary, L2[5], seq_len, bwt_size, n_sa;
  int32_t sa_intv, pad_;
} bpsw_fmi_shape_t;
int bpsw_fmi_build_shape(int64_t l_pac, int32_t sa_intv, bpsw_fmi_shape_t *shape);
int bpsw_fmi_build(bpsw_ctx_t *ctx, const uint8_t *pac, int64_t l_pac, int32_t sa_intv, int flags, uint32_t *bwt, int64_t bwt_cap,
                   int64_t *sa, int64_t sa_cap, bpsw_fmi_shape_t *out);
void bpsw_last_fmi_build_times(double ms[5]);
void bpsw_last_fmi_build_stats(int64_t st[8]);
void bpsw_fmi_build_set_first_key(int bases);
void bpsw_fmi_build_set_budget(int64_t bytes);

/* ---- worker2's tail: everything after the rescue ------------------------------------------
 *
 * memSamPeGroupRest (worker2/MemSamPe.scala:1390-1612 == mem_sam_pe after the rescue, native/bwamem_pair.c:385-452):
 * memMarkPrimarySe, memPair, the mapQ arithmetic, memRegToAln (band inference, up to three banded global alignments,
 * NM/MD, position, clipping) and the SAM text (memAlnToSAM, worker2/MemRegToADAMSAM.scala:328-560).  Not behind either
 * JNI of the reference (the Scala calls them directly), so these are additional exports like bpsw_global_batch.
 * The global alignments, NM/MD and the coordinates run on the GPU against the reference loaded with bpsw_ref_load
 * (bpsw_reg2aln.hip); the per-pair bookkeeping and the text are host code (bpsw_tail.cpp).
 *
 * flavour: where the Scala text and the C it was transcribed from differ (band rule of bwaGenCigar2,
 * mapQ at len == mapQCoefLen, hash ordering and parent index in memMarkPrimarySe, flag folding in memAlnToSAM) the
 * Scala form is BPSW_TAIL_SCALA (default) and the C form BPSW_TAIL_C.
 */
#define BPSW_TAIL_SCALA 0
#define BPSW_TAIL_C 1
#define BPSW_MEM_F_NOPAIRING 0x4 /* bits of bpsw_opt_t.flag the tail reads (native/bwamem.h:14-19) */
#define BPSW_MEM_F_ALL 0x8
#define BPSW_MEM_F_NO_MULTI 0x10
#define BPSW_R2A_MAX_QLEN 1024 /* read length */
#define BPSW_R2A_MAX_RLEN 4096 /* re - rb of a region */
/* The two limits above are tested per job; together they are bounded by the kernel's staging of one job per wavefront in LDS.
 * With Q = the longest read and R = the longest region (re - rb) of a launch, each rounded up to a multiple of 32, a launch
 * passes when 16 Q + 2 R + 2096 <= 16384, i.e. 8 Q + R <= 7144, and is refused with BPSW_ERR_LIMIT otherwise (one long job
 * refuses its whole call).  So: reads up to 352 bases go with regions up to 4096; 512 with 3040; 640 with 2016; 768 with 992;
 * 864 with 224; reads of 865 bases and more are always refused, BPSW_R2A_MAX_QLEN notwithstanding. */

typedef struct { /* the MemOptType fields only the tail reads (datatype/MemOptType.scala:47-52) */
  float mask_level, mapq_coef_len;
  int32_t mapq_coef_fac;
  int32_t flavour;
  char rg_id[64]; /* read-group ID ("" = none): every SAM line gets \tRG:Z:<id> behind XS (worker2/MemRegToADAMSAM.scala:496-500 ==
                     native/bwamem.c:815; the ID is what SAMHeader.bwaSetReadGroup / bwa_set_rg cut out of the -R line) */
} bpsw_tail_opt_t;
void bpsw_tail_opt_default(bpsw_tail_opt_t *t);

/* The contig table of the reference loaded with bpsw_ref_load (bntann1_t offset / len / name, native/bntseq.h:40-46 ==
 * datatype/BNTSeqType.scala); shared by every context of the device like the reference itself.  names: n_seqs
 * NUL-terminated strings back to back, or NULL (then the SAM text uses "ctgN"). */
int bpsw_bns_load(bpsw_ctx_t *ctx, int32_t n_seqs, const int64_t *offset, const int32_t *len, const char *names);

#define BPSW_ALN_OK 0
#define BPSW_ALN_XREF 1     /* bwaFixXref2 could not repair the hit (the Scala asserts, R2S:196-199; the C exits) */
#define BPSW_ALN_NOCIGAR 2  /* bwaGenCigar2 returned null (window out of range / bridging the strands) */
#define BPSW_ALN_OVERFLOW 3 /* more CIGAR operations / MD bytes than the kernel stages: not produced */
typedef struct { /* MemAlnType (datatype/MemAlnType.scala) == mem_aln_t (native/bwamem.h:71-80); CIGAR and MD beside it */
  int64_t pos;
  int32_t rid, flag, is_rev, mapq, NM, n_cigar, score, sub, md_len, status;
} bpsw_aln_t; /* 48 bytes */

/* memRegToAln (worker2/MemRegToADAMSAM.scala:172-313 == mem_reg2aln, native/bwamem.c:949-1021) for n (read, region) jobs.
 * regs[j].rb < 0 or .re < 0: the unmapped record.  out_cigar: max_cigar words per job (len<<4|op, op MIDS=0123);
 * out_md: max_md bytes per job (text, no NUL).  A job whose n_cigar > max_cigar or md_len > max_md has to be resubmitted
 * with more room (nothing is truncated silently: its status is BPSW_ALN_OVERFLOW only past the kernel's own staging). */
typedef struct {
  int32_t n;
  int32_t max_cigar, max_md;
  const int32_t *read_len;
  const int64_t *read_off;
  const uint8_t *read_pool; /* codes 0..4 */
  size_t read_pool_bytes;
  const bpsw_alnreg_t *regs;
} bpsw_reg2aln_jobs_t;
int bpsw_reg2aln_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, const bpsw_reg2aln_jobs_t *jobs,
                       bpsw_aln_t *out, uint32_t *out_cigar, uint8_t *out_md);

/* The tail over a group of pairs.  Arrays are indexed 2k+i (pair k, end i); regions in (k, i, j) order as
 * bpsw_matesw_group leaves them.  id0: pair id of the first pair (the reference hashes id0 + k).
 * Output: out_text receives the SAM lines (read 2k+i: out_text[out_off[2k+i] .. out_off[2k+i+1]); a read with
 * supplementary hits has several lines); BPSW_ERR_CAPACITY with *out_needed set when text_cap is too small (out_text then
 * holds a part of the text, nothing is written past text_cap, out_off is complete: call again with *out_needed bytes).
 * out_regs (optional, same size as regs): the region lists as the tail leaves them (sorted, sub/sub_n/secondary/hash). */
typedef struct {
  int32_t group_size;
  int64_t id0;
  bpsw_pestat_t pes[4];
  const int32_t *read_len;
  const int64_t *read_off;
  const uint8_t *read_pool;
  const uint8_t *qual_pool; /* same offsets as read_pool, or NULL */
  size_t read_pool_bytes;
  const int64_t *name_off;  /* group_size + 1 offsets into name_pool */
  const char *name_pool;
  const int32_t *reg_cnt;
  const bpsw_alnreg_t *regs;
} bpsw_pairs_t;
int bpsw_sam_pe_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, const bpsw_pairs_t *g, char *out_text,
                      size_t text_cap, int64_t *out_off, size_t *out_needed, bpsw_alnreg_t *out_regs);
/* Host-only pieces of the tail and of the rescue bookkeeping, exported so that they can be used and tested without a device
 * (no context, no GPU): memMarkPrimarySe (sorts regs in place and fills sub / sub_n / secondary / hash), memApproxMapqSe,
 * memPair (out5 = {score, sub, n_sub, z0, z1}) and memSortAndDedup (mode BPSW_RESCUE_C / _SCALA; returns the new count). */
int bpsw_mark_primary_se(const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, int32_t n, bpsw_alnreg_t *regs, int64_t id);
int bpsw_approx_mapq_se(const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, const bpsw_alnreg_t *reg);
int bpsw_mem_pair(const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, int64_t l_pac, const bpsw_pestat_t pes[4], int32_t n0,
                  const bpsw_alnreg_t *regs0, int32_t n1, const bpsw_alnreg_t *regs1, int64_t id, int32_t out5[5]);
int bpsw_sort_dedup(int32_t n, bpsw_alnreg_t *regs, float mask_level_redun, int mode);
/* HARNESS ONLY -- outside both boundaries (the driver's job), kept because the tests and tools that build worker2
 * inputs need the pes[] the driver would have computed; a maintainer wiring the library into the aligner does not bind it.
 * memPeStat (worker2/MemSamPe.scala:117-260 == mem_pestat, native/bwamem_pair.c:50-112): the insert-size statistics the driver
 * computes between worker1 and worker2, from the region lists of n_pairs pairs in (pair, end, j) order.  Nothing is printed. */
int bpsw_pe_stat(const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, int64_t l_pac, int32_t n_pairs, const int32_t *reg_cnt,
                 const bpsw_alnreg_t *regs, bpsw_pestat_t pes[4]);

/* worker2 in one call: the rescue of boundary 1 (anchors and windows as memSamPeGroupJNIPrepare builds them,
 * worker2/MemSamPe.scala:1895-2000, windows named by coordinates of the reference loaded with bpsw_ref_load; rescue_mode as in
 * bpsw_matesw_group) followed by the tail above.  g->regs are the region lists BEFORE the rescue (what worker1 hands over).
 * out_reg_cnt (2*group_size, optional) / out_regs (optional): the lists after the rescue and the tail's bookkeeping. */
int bpsw_worker2_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, const bpsw_pairs_t *g, int rescue_mode,
                       char *out_text, size_t text_cap, int64_t *out_off, size_t *out_needed, int32_t *out_reg_cnt,
                       bpsw_alnreg_t *out_regs, int64_t out_regs_cap, int64_t *out_regs_total);
/* The tail off the calling thread: a library-owned pool of n_workers tail workers on one device (each with a context of its own).
 * The reference runs memSamPeGroupRest in the partition's task thread (worker2/MemSamPe.scala:1390-1612 under FastMap.scala:266-293);
 * with the pool that thread only ENQUEUES its groups and collects the text later -- plan, kernel and text of different groups overlap.
 * bpsw_tail_pool_submit copies opt, topt and *g by value and returns a ticket at once; everything they and the out_* arguments point
 * to stays the caller's and must stay valid and unchanged until the ticket is collected.  rescue_mode: BPSW_RESCUE_C / BPSW_RESCUE_SCALA
 * = bpsw_worker2_batch (rescue + tail), BPSW_TAIL_POOL_TAIL_ONLY = bpsw_sam_pe_batch (out_reg_cnt / out_regs_cap unused; out_regs as
 * there).  bpsw_tail_pool_wait blocks until the ticket's group is done and returns ITS return code (BPSW_ERR_CAPACITY with *out_needed /
 * *out_regs_total set, exactly as the direct calls; the worker's error text becomes the collecting thread's bpsw_last_error());
 * tickets may be collected in any order, each once.  bpsw_tail_pool_destroy runs what is still queued, then joins the workers. */
typedef struct bpsw_tail_pool bpsw_tail_pool_t;
#define BPSW_TAIL_POOL_TAIL_ONLY (-1)
int bpsw_tail_pool_create(int device, int n_workers, bpsw_tail_pool_t **out);
void bpsw_tail_pool_destroy(bpsw_tail_pool_t *pool);
int bpsw_tail_pool_submit(bpsw_tail_pool_t *pool, const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, const bpsw_pairs_t *g,
                          int rescue_mode, char *out_text, size_t text_cap, int64_t *out_off, int32_t *out_reg_cnt,
                          bpsw_alnreg_t *out_regs, int64_t out_regs_cap, int64_t *ticket);
int bpsw_tail_pool_wait(bpsw_tail_pool_t *pool, int64_t ticket, size_t *out_needed, int64_t *out_regs_total);
int bpsw_tail_pool_workers(const bpsw_tail_pool_t *pool);
/* the most recent tail call on this context: kernel_ms = reg2aln_kernel launches (hipEvents on the launch stream), n_jobs =
 * jobs they carried, host_ms = {plan, device round trip (staging, copies, kernel), emit} of bpsw_sam_pe_batch */
int bpsw_last_tail_times(bpsw_ctx_t *ctx, float *kernel_ms, int32_t *n_jobs, double host_ms[3]);
/* ... and how many of its jobs were launched again because their CIGAR or MD outgrew the room of the launch before (the tail gives
 * every job room for 16 operations / 64 MD bytes first, then 128 / 512, then 514 / 4096; a job is counted once per extra launch) */
int bpsw_last_tail_resubmitted(bpsw_ctx_t *ctx, int32_t *n_resubmitted);

/* ---- single-end reads to SAM (bpsw_sam_se.hip) ---------------------------------------------------------------------------
 *
 * bpsw_sam_se_batch is singleEndBwaMemWorker2 (worker2/BWAMemWorker2.scala:49-58 == native/bwamem.c:1052-1056) for a batch: per read
 * mem_mark_primary_se with id = id0 + r * id_step, then mem_reg2sam_se with extra_flag = 0 and no mate (native/bwamem.c:879-892 ==
 * memRegToSAMSe, worker2/MemRegToADAMSAM.scala:67-118): regions with score >= T, secondary hits only under BPSW_MEM_F_ALL and not
 * below half their parent's score, one memRegToAln job each (on the GPU, as in the paired tail), 0x800 (0x10000 under
 * BPSW_MEM_F_NO_MULTI) for later primaries, their mapQ capped at the first line's, the unaligned record for a read without a
 * selected region, and the SAM lines without the mate's flag bits and with "*\t0\t0" for the mate columns.  id_step: 1 is the C
 * (n_processed + i), 0 is what FastMap.scala:624-635 does (every read of a batch gets the same numProcessed); any value >= 0.
 * Both flavours and topt->rg_id as in bpsw_sam_pe_batch; text, out_off (n_reads + 1), *out_needed and BPSW_ERR_CAPACITY as there
 * (nothing is written past text_cap, out_off is complete); BPSW_ERR_LIMIT where the reference aborts (XREF) or an alignment
 * outgrows the kernel's CIGAR staging; BPSW_ERR_ARG for a read outside its pool or an empty read; bpsw_reg2aln_batch's size limits;
 * n_reads == 0 is fine.  out_regs (optional, same size as regs): the lists after mem_mark_primary_se.  Fills
 * bpsw_last_tail_times as the paired tail does.
 *
 * flags: with BPSW_SAM_TEXT_DEVICE the text is written by two kernels (the length of every line, then its bytes, one line per
 * lane) and comes back in one copy; the bytes are the same.  Default: on the calling thread, as in the paired tail (which has
 * the same flag in bpsw_sam_pe_batch_ex, below).
 *
 * bpsw_align_se_batch is FastMap.scala:624-625 in one call: bpsw_worker1_batch with w1_flags | BPSW_C2A_SORT_DEDUP and zdrop_mode
 * (its capacity retry handled inside), then bpsw_sam_se_batch on the lists it got (g->reg_cnt / g->regs are ignored).  Needs the
 * reference, the contig table and the index on the context's device; reads of at most BPSW_SEED_MAX_QLEN bases. */
#define BPSW_SAM_TEXT_DEVICE 1 /* flags: write the SAM text on the device; default: on the calling thread */
typedef struct {
  int32_t n_reads;
  int64_t id0;
  int32_t id_step; /* read r is hashed as id0 + r * id_step (mem_mark_primary_se's id) */
  const int32_t *read_len;
  const int64_t *read_off;
  const uint8_t *read_pool; /* codes 0..4 */
  const uint8_t *qual_pool; /* same offsets as read_pool, or NULL ('*') */
  size_t read_pool_bytes;
  const int64_t *name_off; /* n_reads + 1 offsets into name_pool */
  const char *name_pool;
  const int32_t *reg_cnt; /* worker1's lists, read order; ignored by bpsw_align_se_batch */
  const bpsw_alnreg_t *regs;
} bpsw_se_reads_t;
int bpsw_sam_se_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, const bpsw_se_reads_t *reads, int flags,
                      char *out_text, size_t text_cap, int64_t *out_off, size_t *out_needed, bpsw_alnreg_t *out_regs);
int bpsw_align_se_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt,
                        const bpsw_se_reads_t *reads, int zdrop_mode, int w1_flags, int flags, char *out_text, size_t text_cap,
                        int64_t *out_off, size_t *out_needed);
/* Diagnostics, of the calling thread's most recent call of the two above (ms): sam_len_kernel, sam_write_kernel (0 without
 * BPSW_SAM_TEXT_DEVICE), building and staging the line table, the round trip of the two kernels with the copies; and of
 * bpsw_align_se_batch: its bpsw_worker1_batch stage, its bpsw_sam_se_batch stage. */
void bpsw_last_sam_se_times(double ms[6]);

/* ---- paired-end reads to SAM (bpsw_sam_pe.hip) ------------------------------------------------------------------------------
 *
 * bpsw_sam_pe_batch_ex is bpsw_sam_pe_batch with a flags argument.  flags == 0 IS bpsw_sam_pe_batch.  With BPSW_SAM_TEXT_DEVICE
 * the text is written by the two kernels of the single-end text (the length of every line, then its bytes, one line per lane):
 * every line carries the index of the first line of its pair's other read, from which the kernels take what memAlnToSAM reads of
 * the mate -- contig, position, strand and the CIGAR's length on the reference, for the flag bits 0x8 / 0x20, the position an
 * unmapped end is placed at, RNEXT, PNEXT and TLEN.  The bytes are the same.  The contract is bpsw_sam_pe_batch's: out_off
 * (2 * group_size + 1), *out_needed with BPSW_ERR_CAPACITY (nothing written past text_cap, out_off complete), BPSW_ERR_LIMIT,
 * group_size == 0, out_regs, bpsw_last_tail_times.  A flag other than BPSW_SAM_TEXT_DEVICE is BPSW_ERR_ARG.
 *
 * bpsw_align_pe_batch is mem_process_seqs under MEM_F_PE (native/bwamem.c:1064-1083 == FastMap.scala:262-307 and :352-395) for a
 * batch of pairs, in one call: bpsw_worker1_batch on the 2 * group_size reads with w1_flags | BPSW_C2A_SORT_DEDUP and zdrop_mode
 * (its capacity retry handled inside); the insert-size statistics -- pes0[4] when given (the reference's pes0), else bpsw_pe_stat
 * over this batch's lists -- returned through out_pes[4] when that is not NULL; the rescue of bpsw_worker2_batch with
 * rescue_mode; bpsw_sam_pe_batch_ex with flags.  g->reg_cnt, g->regs and g->pes are ignored; pair k is hashed as g->id0 + k.
 * Needs the reference, the contig table and the index on the context's device.  The refusals are the stages': a read of more than
 * BPSW_SEED_MAX_QLEN bases is BPSW_ERR_LIMIT, no index (or no reference) BPSW_ERR_ARG; group_size == 0 is fine. */
int bpsw_sam_pe_batch_ex(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, const bpsw_pairs_t *g, int flags,
                         char *out_text, size_t text_cap, int64_t *out_off, size_t *out_needed, bpsw_alnreg_t *out_regs);
int bpsw_align_pe_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt,
                        const bpsw_pairs_t *g, const bpsw_pestat_t *pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags,
                        char *out_text, size_t text_cap, int64_t *out_off, size_t *out_needed, bpsw_pestat_t *out_pes);
/* Diagnostics, of the calling thread's most recent call of the two above (ms): sam_len_kernel, sam_write_kernel (0 without
 * BPSW_SAM_TEXT_DEVICE), building and staging the line table, the round trip of the two kernels with the copies; and of
 * bpsw_align_pe_batch: its worker1 stage, the statistics, the rescue, the tail. */
void bpsw_last_sam_pe_times(double ms[8]);

/* ---- FASTQ text to reads, and FASTQ text to SAM text (bpsw_fastq.hip) --------------------------------------------------------
 *
 * bpsw_fastq_parse turns a chunk of four-line FASTQ text in memory into the form the entries above take: base codes 0..4 and
 * qualities in two pools at the same offsets, read_len / read_off (one entry per read), names in a pool with name_off (one more
 * entry than names).  The record rules are csrc/bpsw_fastq_core.h's and follow the reference's C (kseq_read and bseq_read with
 * trim_readno): a line ends at '\n' and loses one '\r' in front of it when it has more than one byte; line 4r begins with '@', line
 * 4r + 2 with '+' (its rest is ignored), line 4r + 3 is as long as line 4r + 1, which is not empty; the name is what follows '@' up
 * to the first isspace byte, without a trailing "/" + digit when it is longer than 2 bytes, and not empty; Aa Cc Gg Tt are 0..3 and
 * every other base is 4, except '-' and bytes below 4, which are refused; qualities are copied.  Multi-line records, blank lines
 * between records and the comment field are not handled (the first two are refused as "not four-line FASTQ"); compressed text is the
 * bpsw_fastq_bgzf_* entries' (BGZF blocks; plain gzip is not handled).
 *
 * text1 / bytes1, text2 / bytes2: one text (text2 NULL, bytes2 0), or the two texts of paired reads -- record k of text1 is read 2k,
 * record k of text2 read 2k + 1, as bseq_read interleaves them.  Only whole records are parsed: consumed[i] is the offset just
 * behind the last parsed record of text i + 1, for the caller to carry the remainder into its next chunk.  With two texts the number
 * of records is the smaller of the two, and both consumed values stop there.  An empty text is *n_reads == 0.  flags:
 *   BPSW_FASTQ_FINAL        the text ends here: a last line without '\n' counts as a line, and a trailing part that is still not a
 *                           whole record is refused.  Without it such a part is just left unconsumed.
 *   BPSW_FASTQ_INTERLEAVED  one text whose records alternate between the two ends; an odd record count leaves the last unconsumed.
 *   BPSW_FASTQ_PAIR_NAMES   one name per pair, the first end's (what bpsw_pairs_t takes); the second end's name, after the same
 *                           rules, must equal it.  Implied by two texts; with one text it needs BPSW_FASTQ_INTERLEAVED.
 *   BPSW_FASTQ_HOST         apply the same rules serially on the calling thread: nothing is launched, ctx may be NULL.
 * Any other flag is BPSW_ERR_ARG.  Capacities: read_len and read_off have max_reads entries, name_off max_reads + 1, the two pools
 * pool_cap bytes each, name_pool name_cap bytes.  When any of them is too small the call returns BPSW_ERR_CAPACITY with needed[3] =
 * {reads, pool bytes, name bytes} of this text, all three, and writes nothing; needed is also set when the call succeeds.  A
 * malformed record is BPSW_ERR_ARG and wins over a capacity: the call reports the lowest such read, and the error text names the
 * entry, the record, the text (1 or 2) and the reason.  A text of 2^31 bytes or more is BPSW_ERR_LIMIT.
 *
 * bpsw_align_fastq_se / bpsw_align_fastq_pe: the parse, then bpsw_align_se_batch / bpsw_align_pe_batch on its result, in one call.
 * fastq_flags are the parse's (the paired entry takes two texts, or one with BPSW_FASTQ_INTERLEAVED; one name per pair either way);
 * every other argument, the text contract (out_text, text_cap, out_off, *out_needed, BPSW_ERR_CAPACITY) and the refusals are the
 * align entry's.  Single-end reads are hashed as id0 + r * id_step, pairs as id0 + k.  out_off has max_reads + 1 entries: a text
 * with more reads is BPSW_ERR_CAPACITY with *n_reads set.  *n_reads and consumed come back as from the parse. */
#define BPSW_FASTQ_FINAL 1
#define BPSW_FASTQ_INTERLEAVED 2
#define BPSW_FASTQ_PAIR_NAMES 4
#define BPSW_FASTQ_HOST 8
int bpsw_fastq_parse(bpsw_ctx_t *ctx, const char *text1, size_t bytes1, const char *text2, size_t bytes2, int flags, int64_t max_reads,
                     size_t pool_cap, size_t name_cap, int32_t *read_len, int64_t *read_off, uint8_t *read_pool, uint8_t *qual_pool,
                     int64_t *name_off, char *name_pool, int64_t *n_reads, int64_t consumed[2], int64_t needed[3]);
int bpsw_align_fastq_se(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt,
                        const char *text, size_t bytes, int fastq_flags, int64_t id0, int32_t id_step, int zdrop_mode, int w1_flags,
                        int flags, char *out_text, size_t text_cap, int64_t *out_off, int64_t max_reads, size_t *out_needed,
                        int64_t *n_reads, int64_t *consumed);
int bpsw_align_fastq_pe(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt,
                        const char *text1, size_t bytes1, const char *text2, size_t bytes2, int fastq_flags, int64_t id0,
                        const bpsw_pestat_t *pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags, char *out_text,
                        size_t text_cap, int64_t *out_off, int64_t max_reads, size_t *out_needed, bpsw_pestat_t *out_pes,
                        int64_t *n_reads, int64_t consumed[2]);
/* Diagnostics, of the calling thread's most recent parse (ms): fastq_count_kernel, fastq_lines_kernel, fastq_record_kernel,
 * fastq_emit_kernel (events on the stream around each; 0 under BPSW_FASTQ_HOST), and the parse's round trip with the copies. */
void bpsw_last_fastq_times(double ms[5]);

/* ---- alignments out as BAM (bpsw_bam.hip) -----------------------------------------------------------------------------------------
 *
 * Every entry above that writes SAM text on the device has a twin that writes the same lines as BAM records (SAM specification 4.2),
 * framed as BGZF blocks: bpsw_bam_se_batch / bpsw_bam_pe_batch are bpsw_sam_se_batch / bpsw_sam_pe_batch_ex, bpsw_align_bam_*_batch
 * are bpsw_align_*_batch, bpsw_align_fastq_bam_* are bpsw_align_fastq_* -- the same bodies with the other writer.  The record of a line
 * holds what the line says (csrc/bpsw_bam_core.h: refID, pos, bin, the folded flag, the CIGAR with H for S on later lines, SEQ two bases a
 * byte, QUAL - 33 or 0xff, NM MD AS XS RG SA in the text's order, integers in the narrowest type).  The records of a call, in line
 * order, form one stream of S bytes that is cut every P bytes (P = 65280 unless bpsw_bam_set_block_payload says otherwise; records
 * do not respect the cuts) into ceil(S / P) gzip members of one STORED deflate block each -- nothing is compressed -- with the CRC-32
 * computed on the device.  out receives S + 31 ceil(S / P) bytes: a whole number of BGZF blocks, so that
 *     bpsw_bam_header || the outputs of any number of calls || bpsw_bam_eof
 * is a valid BAM file.  There is no out_off: a record carries its own length.  BPSW_ERR_CAPACITY with *out_needed set when cap is too
 * small (nothing is written then: the size is known before the records are); an empty batch is *out_needed == 0.  flags must be 0
 * (BPSW_ERR_ARG otherwise); the FASTQ twins keep fastq_flags, and w1_flags pass through.  A read name of more than 254 bytes cannot be
 * a BAM record: BPSW_ERR_LIMIT, nothing written.  Everything else -- arguments, refusals, out_regs, out_pes, n_reads, consumed,
 * bpsw_last_tail_times -- is the twin's.  Sorting and an index: bpsw_bam_sort, below.
 *
 * flags = BPSW_BAM_DEFLATE (all six entries; any other bit is still BPSW_ERR_ARG): every member holds one dynamic-Huffman deflate block
 * with LZ77 matches (RFC 1951, BTYPE 10), made on the device by one wavefront a block (csrc/bpsw_deflate_core.h), unless that would not
 * be smaller than the stored form, which the member then keeps: no member grows.  The records, the cuts, the CRC-32 and ISIZE are the
 * same, and the bytes are a function of the stream and P alone.  The size is known only after compression: with cap too small (or out
 * NULL) the call still compresses, writes nothing and returns BPSW_ERR_CAPACITY with *out_needed the exact size, at which a repeat
 * succeeds.  A caller who wants one call sizes by the stored form, S + 31 ceil(S / P) -- what the same call with flags == 0 reports --
 * which the compressed output never exceeds.  Outputs with and without the flag concatenate; the header and the EOF block are as before. */
#define BPSW_BAM_DEFLATE 16 /* flags: compress every BGZF block on the device; default: stored blocks */
int bpsw_bam_se_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, const bpsw_se_reads_t *reads, int flags, char *out,
                      size_t cap, size_t *out_needed, bpsw_alnreg_t *out_regs);
int bpsw_bam_pe_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_tail_opt_t *topt, const bpsw_pairs_t *g, int flags, char *out,
                      size_t cap, size_t *out_needed, bpsw_alnreg_t *out_regs);
int bpsw_align_bam_se_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt,
                            const bpsw_se_reads_t *reads, int zdrop_mode, int w1_flags, int flags, char *out, size_t cap,
                            size_t *out_needed);
int bpsw_align_bam_pe_batch(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt,
                            const bpsw_pairs_t *g, const bpsw_pestat_t *pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags,
                            char *out, size_t cap, size_t *out_needed, bpsw_pestat_t *out_pes);
int bpsw_align_fastq_bam_se(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt,
                            const char *text, size_t bytes, int fastq_flags, int64_t id0, int32_t id_step, int zdrop_mode, int w1_flags,
                            int flags, char *out, size_t cap, size_t *out_needed, int64_t *n_reads, int64_t *consumed);
int bpsw_align_fastq_bam_pe(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt,
                            const char *text1, size_t bytes1, const char *text2, size_t bytes2, int fastq_flags, int64_t id0,
                            const bpsw_pestat_t *pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags, char *out, size_t cap,
                            size_t *out_needed, bpsw_pestat_t *out_pes, int64_t *n_reads, int64_t consumed[2]);
/* The header, on the calling thread (nothing is launched).  bpsw_sam_header: the text "@HD\tVN:1.6\tSO:unsorted\n", one
 * "@SQ\tSN:<name>\tLN:<len>\n" per contig, then `extra` (extra_bytes of the caller's own lines, @RG / @PG, verbatim; NULL for none).
 * The contigs are those loaded with bpsw_bns_load when ctx is given (n_seqs, len and names are ignored), else the table of the
 * arguments: len[n_seqs] and names as bpsw_bns_load takes them (NULL: no names).  A contig without a name is "ctg<rid + 1>", as in the
 * lines.  bpsw_bam_header: "BAM\1", l_text, that text, n_ref and per contig l_name, the name with its NUL and l_ref, framed as BGZF
 * blocks like the records.  bpsw_bam_eof: the 28-byte end-of-file block of the specification.  All three: BPSW_ERR_CAPACITY with
 * *out_needed set, and nothing written, when cap is too small.
 * The two with _ex take flags behind extra_bytes: BPSW_HDR_COORDINATE writes "SO:coordinate" where the plain entries write
 * "SO:unsorted" (for what bpsw_bam_sort made); 0 gives the plain entries' bytes, which are calls of these with 0; any other bit is
 * BPSW_ERR_ARG. */
#define BPSW_HDR_COORDINATE 1
int bpsw_sam_header_ex(bpsw_ctx_t *ctx, int32_t n_seqs, const int32_t *len, const char *names, const char *extra, size_t extra_bytes,
                       int flags, char *out, size_t cap, size_t *out_needed);
int bpsw_bam_header_ex(bpsw_ctx_t *ctx, int32_t n_seqs, const int32_t *len, const char *names, const char *extra, size_t extra_bytes,
                       int flags, char *out, size_t cap, size_t *out_needed);
int bpsw_sam_header(bpsw_ctx_t *ctx, int32_t n_seqs, const int32_t *len, const char *names, const char *extra, size_t extra_bytes, char *out,
                    size_t cap, size_t *out_needed);
int bpsw_bam_header(bpsw_ctx_t *ctx, int32_t n_seqs, const int32_t *len, const char *names, const char *extra, size_t extra_bytes, char *out,
                    size_t cap, size_t *out_needed);
int bpsw_bam_eof(char *out, size_t cap, size_t *out_needed);
/* The payload bytes of a BGZF block, process-wide: 1 .. 65280; 0 = the default, 65280 (htslib's).  Anything else is BPSW_ERR_ARG and
 * changes nothing.  The counterpart of bpsw_scan_set_tile: tests put block edges anywhere in a small batch with it. */
int bpsw_bam_set_block_payload(int bytes);
/* Diagnostics, of the calling thread's most recent call of a BAM entry (ms): bam_len_kernel, bam_write_kernel, bgzf_frame_kernel,
 * building and staging the line table, the round trip of the three kernels with the copies. */
void bpsw_last_bam_times(double ms[5]);
/* ... and of what BPSW_BAM_DEFLATE adds (ms; zeros after a call without it): bgzf_deflate_kernel, bgzf_pack_kernel (0 when the capacity
 * was refused), the blocks' size table back to the host with its sum and the offsets' way out, the copy of the packed blocks.  With the
 * flag, slot 2 of bpsw_last_bam_times (bgzf_frame_kernel) is 0. */
void bpsw_last_bam_deflate_times(double ms[4]);

/* ---- a coordinate-sorted BAM and its .bai: the records sorted on the device (bpsw_bam_sort.hip) -----------------------------------------
 * in[0, in_bytes): what the BAM entries return, concatenated -- a whole number of BGZF blocks (stored or deflated in any mix; whatever
 * bpsw_bgzf_inflate accepts, under its rules and refusals; empty blocks such as bpsw_bam_eof's may stand anywhere) whose inflated bytes
 * are a whole number of BAM records.  A header is not accepted: the caller has it and puts it in front.
 * seg_off[n_seg]: optional.  Offsets into `in`, ascending, each on a block boundary (0 and in_bytes are boundaries), at which a record
 * is known to begin -- where the calls' outputs begin, or end.  They cut the input into n_seg + 1 segments: segment 0 from 0 to
 * seg_off[0], segment k from seg_off[k - 1] to seg_off[k], the last one to in_bytes.  The one serial step, following block_size from
 * record to record, then runs once per segment, side by side.  n_seg == 0: the whole input is one segment.  Two equal offsets, or a
 * first one of 0, or a last one of in_bytes, are an empty segment.  An offset that is no block boundary, or a segment whose chain of
 * block_size fields does not end exactly on the segment's end, is BPSW_ERR_ARG; the text names the segment and the offset in the
 * inflated stream.
 * The contigs: len[n_seqs] when len is given; with len NULL those of the table loaded with bpsw_bns_load on ctx's device (n_seqs is
 * ignored then; no table and n_seqs != 0 is BPSW_ERR_ARG).  They must be the header's.
 *
 * The order -- this library's definition of SO:coordinate, which the specification leaves open beyond (refID, pos) with the reads
 * without a coordinate last: the key is (refID, pos + 1, flag bit 0x10), a refID of -1 counting as n_seqs; records of equal keys keep
 * the order they have in `in` (the sort is stable).  So at one position the forward strand stands before the reverse strand, and an
 * input that is sorted comes back as it is.  The records' bytes are not changed (the bin field included).
 *
 * out: the sorted stream cut every P bytes (bpsw_bam_set_block_payload) and framed as the BAM entries frame theirs -- stored, or with
 * flags = BPSW_BAM_DEFLATE compressed on the device -- so that  bpsw_bam_header_ex(BPSW_HDR_COORDINATE) || out || bpsw_bam_eof  is a
 * sorted BAM file.  bai: its index (specification 5.2) for a file in which `out` begins at byte file_off (the header's size): per
 * contig the bins in ascending order with their chunks in file order -- a chunk is a maximal run of consecutive records with the same
 * bin, the bin recomputed from pos and the CIGAR; then the pseudo-bin 37450; the linear index (a 16 Kib window's entry is the start of
 * the first record that overlaps it, a window that none overlaps takes the next one's, n_intv is the last overlapped window + 1);
 * a contig without records has n_bin = n_intv = 0; n_no_coor at the end.  *n_records: the records.
 * Capacity: as for the BAM entries, for both buffers together.  When cap or bai_cap is too small (or the buffer NULL) the call does
 * all its work, writes nothing to either and returns BPSW_ERR_CAPACITY with *out_needed and *bai_needed exact; a repeat at those
 * sizes succeeds.
 * Refusals, with the first offending record named by its index in the input stream: in_bytes or the inflated size at 2^31 or above, or
 * a contig longer than 2^29 (a BAI cannot bin it): BPSW_ERR_LIMIT.  A refID outside [-1, n_seqs); a pos below -1, or at or above its
 * contig's length (a record with refID -1 has no contig: its pos is -1); a block_size below 32 + l_read_name + 4 n_cigar_op +
 * ceil(l_seq / 2) + l_seq: BPSW_ERR_ARG.  Not here: merging the sorted outputs of several calls, CSI, other orders. */
int bpsw_bam_sort(bpsw_ctx_t *ctx, const char *in, size_t in_bytes, const int64_t *seg_off, int64_t n_seg, int32_t n_seqs,
                  const int32_t *len, int64_t file_off, int flags, char *out, size_t cap, size_t *out_needed, char *bai, size_t bai_cap,
                  size_t *bai_needed, int64_t *n_records);
/* The bytes of the stream a wavefront of bam_walk_kernel holds in LDS, process-wide: 64 .. 16384, rounded up to a multiple of 16;
 * 0 = the default, 4096.  Anything else is BPSW_ERR_ARG and changes nothing.  The counterpart of bpsw_bam_set_block_payload: tests put
 * the window's edge inside every part of a record with it. */
int bpsw_bam_sort_set_window(int bytes);
/* Diagnostics, of the calling thread's most recent bpsw_bam_sort (ms): bgzf_inflate_kernel, bam_walk_kernel (both passes and the scan
 * between them), bam_key_kernel, the radix sort, the lengths' gather with its scan and bam_gather_kernel, bgzf_frame_kernel or
 * bgzf_deflate_kernel with bgzf_pack_kernel, the index table's way back with the BAI's assembly, the call's round trip. */
void bpsw_last_bam_sort_times(double ms[8]);

/* ---- FASTQ in as BGZF: the blocks inflated on the device, parsed from there (bpsw_bgzf_in.hip, bpsw_fastq.hip) ------------------------
 * Accepted: a sequence of BGZF blocks -- gzip members that begin 1f 8b 08 04 and whose extra field has the subfield BC (SLEN 2) with
 * BSIZE; other subfields are skipped.  The deflate data of a block may be anything RFC 1951 allows (any number of stored, fixed and
 * dynamic deflate blocks); the bound is ISIZE <= 65536, and a distance may not reach in front of the block's own output.  A gzip
 * member without BC is refused with BPSW_ERR_ARG ("plain gzip, not BGZF").
 *
 * bpsw_bgzf_inflate: the whole blocks of in[0, in_bytes) to out.  Only whole blocks are inflated: *consumed is the offset behind the
 * last of them, *n_blocks their number, *out_needed the sum of their ISIZE -- all three known from the headers before anything is
 * launched.  cap < *out_needed is BPSW_ERR_CAPACITY with nothing launched.  A malformed header is BPSW_ERR_ARG and wins over a
 * capacity; malformed deflate data, a wrong length or a wrong CRC-32 is BPSW_ERR_ARG too: the lowest such block is reported, and the
 * text names the entry, the block and the reason.  in_bytes or the inflated total at 2^31 or above is BPSW_ERR_LIMIT.  An empty chunk
 * and a lone end-of-file block give *out_needed == 0.
 *   BPSW_BGZF_FINAL   the chunk ends here: bytes behind the last whole block are refused, not left
 *   BPSW_BGZF_HOST    the same rules serially on the calling thread: nothing is launched, ctx may be NULL
 *
 * The five FASTQ entries below are their twins' argument lists with two differences: each text argument is BGZF bytes, and behind
 * each `bytes` comes a `skip`.  The caller's state is a BGZF virtual offset as htslib defines it: skip is the number of inflated bytes
 * of the chunk's first block that earlier calls consumed (0 .. its ISIZE; non-zero without a block, or above it, is BPSW_ERR_ARG), and
 * consumed[i] comes back as coffset << 16 | uoffset: coffset is the chunk offset of the first block whose inflated end lies above the
 * end of the last parsed record, uoffset that end within it; when no such block exists, (the offset behind the last whole block, 0).
 * The next call passes in + coffset and skip = uoffset (it inflates that one block again).  Only whole blocks are read; with
 * BPSW_FASTQ_FINAL a chunk must end on a block boundary ("the text ends inside a BGZF block").  An inflate refusal wins over every
 * refusal of the parse.  On the device the inflated text stays there; with BPSW_FASTQ_HOST it is inflate_serial, then the serial
 * parse, without a context, with identical results and refusals. */
#define BPSW_BGZF_FINAL 1
#define BPSW_BGZF_HOST 2
int bpsw_bgzf_inflate(bpsw_ctx_t *ctx, const char *in, size_t in_bytes, int flags, char *out, size_t cap, size_t *out_needed,
                      int64_t *n_blocks, int64_t *consumed);
/* ms of the calling thread's last bpsw_bgzf_inflate: the header walk, bgzf_inflate_kernel, the round trip with the copies (zeros
 * under BPSW_BGZF_HOST) */
void bpsw_last_bgzf_times(double ms[3]);
int bpsw_fastq_bgzf_parse(bpsw_ctx_t *ctx, const char *text1, size_t bytes1, int32_t skip1, const char *text2, size_t bytes2, int32_t skip2,
                          int flags, int64_t max_reads, size_t pool_cap, size_t name_cap, int32_t *read_len, int64_t *read_off,
                          uint8_t *read_pool, uint8_t *qual_pool, int64_t *name_off, char *name_pool, int64_t *n_reads, int64_t consumed[2],
                          int64_t needed[3]);
int bpsw_align_fastq_bgzf_se(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt, const char *text,
                             size_t bytes, int32_t skip, int fastq_flags, int64_t id0, int32_t id_step, int zdrop_mode, int w1_flags, int flags,
                             char *out_text, size_t text_cap, int64_t *out_off, int64_t max_reads, size_t *out_needed, int64_t *n_reads,
                             int64_t *consumed);
int bpsw_align_fastq_bgzf_pe(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt,
                             const char *text1, size_t bytes1, int32_t skip1, const char *text2, size_t bytes2, int32_t skip2, int fastq_flags,
                             int64_t id0, const bpsw_pestat_t *pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags, char *out_text,
                             size_t text_cap, int64_t *out_off, int64_t max_reads, size_t *out_needed, bpsw_pestat_t *out_pes, int64_t *n_reads,
                             int64_t consumed[2]);
int bpsw_align_fastq_bgzf_bam_se(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt,
                                 const char *text, size_t bytes, int32_t skip, int fastq_flags, int64_t id0, int32_t id_step, int zdrop_mode,
                                 int w1_flags, int flags, char *out, size_t cap, size_t *out_needed, int64_t *n_reads, int64_t *consumed);
int bpsw_align_fastq_bgzf_bam_pe(bpsw_ctx_t *ctx, const bpsw_opt_t *opt, const bpsw_seed_opt_t *sopt, const bpsw_tail_opt_t *topt,
                                 const char *text1, size_t bytes1, int32_t skip1, const char *text2, size_t bytes2, int32_t skip2,
                                 int fastq_flags, int64_t id0, const bpsw_pestat_t *pes0, int zdrop_mode, int w1_flags, int rescue_mode,
                                 int flags, char *out, size_t cap, size_t *out_needed, bpsw_pestat_t *out_pes, int64_t *n_reads,
                                 int64_t consumed[2]);

/* ---- statistics (the buckets of profiling/SWBatchTimeBreakdown.scala:25-39, device flavoured) -- */
typedef struct {
  uint64_t ext_calls, ext_tasks, ext_wire_bytes;
  uint64_t sw_calls, sw_jobs, sw_speculated, sw_replayed_rounds, sw_wasted;
  double ext_h2d_ms, ext_kernel_ms, ext_d2h_ms;
  double sw_h2d_ms, sw_kernel_ms, sw_d2h_ms, sw_host_ms;
  /* wall-clock phases of the host-buffer entry points, summed over calls (ms): staging copy in, waiting for a device
   * stream of the pool, device phase (H2D + kernel + D2H until the stream is idle), staging copy out; for the group
   * rescue: speculation, job packing, waiting, device phase, replay, output copy */
  double ext_host_in_ms, ext_wait_ms, ext_dev_ms, ext_host_out_ms;
  double grp_plan_ms, grp_pack_ms, grp_wait_ms, grp_dev_ms, grp_replay_ms, grp_out_ms;
  uint64_t grp_calls, grp_pairs;
  uint64_t ext_full_relaunches; /* extension calls whose short kernel deferred tasks, so that the full kernel was launched behind it after all */
  uint64_t sw_ring_calls;       /* SW batches that went through the device's submission ring (resident kernel) instead of a launch of their own;
                                   for those sw_kernel_ms is the batch's span on the device clock: first job pair taken -> last one finished */
  uint64_t ext_ring_calls;      /* extension batches (small ones: no long flank, too few tasks for the sift kernel) that went through the
                                   device's extension ring; ext_kernel_ms likewise: first task taken -> last one finished */
} bpsw_stats_t;
int bpsw_get_stats(bpsw_ctx_t *ctx, bpsw_stats_t *out);
int bpsw_reset_stats(bpsw_ctx_t *ctx);
/* duration in ms of the most recent extend / swalign kernel launch on this context, measured with
 * hipEvents on the launch stream.  Synchronises the stream and resolves the asynchronous device entries: their deferred
 * errors are returned here. */
int bpsw_last_kernel_ms(bpsw_ctx_t *ctx, float *ext_ms, float *sw_ms);
/* The submission ring of the context's device (round 5; csrc/bpsw_ring.h): the SW batches of bpsw_swalign2_batch / bpsw_matesw_group /
 * mateSWJNI of ALL contexts of a device are descriptors of one resident kernel instead of launches of their own.  epochs = launches of
 * that kernel (it ends by itself BPSW_RING_IDLE_US after its last batch), submitted = batches appended, carried = batches a closing
 * epoch handed to its successor; epochs_ms / epochs_timed = summed duration and number of the epochs that are OVER, each timed by two HIP
 * events around the resident kernel's launch on its stream (what a kernel trace reports as that kernel's duration).  Diagnostics; any
 * pointer may be null. */
int bpsw_ring_stats(bpsw_ctx_t *ctx, uint64_t *epochs, uint64_t *submitted, uint64_t *carried, double *epochs_ms, uint64_t *epochs_timed);
/* The rings' integrity tripwire (csrc/bpsw_ring.cpp).  A batch's results and its completion word reach host memory as separate writes
 * from many wavefronts; before a caller publishes a batch it poisons every record of its result block with a value no kernel writes, and
 * after the completion word it looks at every record again.  checked = records looked at, faults = records that still held the poison when
 * the completion word was visible (process-wide; expected: 0 -- a fault is reported on stderr once, the call waits up to 5 ms for the
 * records and fails with BPSW_ERR_DEVICE if they do not arrive; an extension batch is run again through a launch instead).  Returns 1
 * when the check is on (default), 0 when BPSW_RING_INTEGRITY=0 switched it off.  Either pointer may be null. */
int bpsw_ring_integrity(uint64_t *checked, uint64_t *faults);
/* A gauge: the number of SW batches (bpsw_swalign2_batch / bpsw_matesw_group / mateSWJNI rounds, of any context) that are in their device
 * phase on `device` right now -- what the "lone caller takes a launch of its own" rule of the SW entry points looks at
 * (BPSW_RING_LONE_LAUNCH).  Diagnostics (an executor's metrics page; tests/test_ring_gpu.py waits on it to make
 * "a batch that has company" a deterministic state instead of a matter of thread timing).  -1 for a device index outside 0..63. */
int bpsw_sw_batches_in_flight(int device);
/* The extension calls that wait for a stream ride one launch chain (csrc/bpsw_ext_group.h; BPSW_EXT_GROUP_MAX).
 * A gauge: the extension calls of the grouped plan (a byte batch behind the sift kernel, results read where the kernel wrote them) that are
 * waiting for a pooled stream of `device` right now; calls that run alone (coordinate batches, the classify entry, rescue launches) wait in the
 * same queue and are not counted.  Diagnostics (tests/test_ext_group_gpu.py waits on it to make "k calls behind one stream" a state instead of a matter of
 * thread timing).  -1 for a device index outside 0..63. */
int bpsw_ext_group_waiting(int device);
/* out[0] = launch chains of the grouped plan so far on `device` (a call that found a free stream is a group of one), out[1] = their members
 * summed, out[2] = the largest group.  Process-wide, never reset. */
int bpsw_ext_group_counts(int device, uint64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif
