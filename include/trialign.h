/*
 * trialign.h -- C-ABI of the MI355X-native three-sequence 3-D DP scorer.
 *
 * This is the drop-in boundary for the reference's one hot path: the TRIALIGN
 * module (timmy139710/HW-Accelerator-Three-Sequence-Alignment), which maps
 * (seqA, seqB, seqC) -> optimal 7-state affine-gap 3-D DP score.
 *
 *   reference interface                        replaced by
 *   ------------------------------------------ ---------------------------------
 *   TRIALIGN ports + parameters                tsa_score_gpu()
 *     src/TriAlign_1cyc.v:1-22                   (lengths A_idx/B_idx/C_idx ->
 *     (start_align pulse, A/B/C_symbol pull,      la/lb/lc; symbol pull protocol
 *      A/B/C_idx lengths, Score, finish)          -> caller-owned byte arrays;
 *                                                 Score/finish -> *score + rc)
 *   PE localparams MATCH/MISMATCH/GO/GE        tsa_params + tsa_default_params()
 *     src/PE_1cyc.v:55-61 (compile-time)         (runtime; defaults = RTL values)
 *   SCORE_BITS parameter (12)                  tsa_params.score_bits
 *     src/TriAlign_tb.sv:56, TriAlign_1cyc.v:6
 *   temp_ABC triple score                      tsa_params.s3_mode (RTL literal by
 *     src/PE_1cyc.v:162                           default; sum-of-pairs optional)
 *   testbench one-shot start/finish FSM        tsa_score_batch(): many triples,
 *     src/TriAlign_tb.sv:279-333                  sharded over the node's GPUs
 *   (no reference equivalent: the reference    tsa_score_batch_async(): device
 *    has one alignment in flight)                 pointers + caller stream, for
 *                                                 in-HBM throughput runs
 *   alignment-output ports (commented out,     tsa_align_gpu(): the optimal path
 *    src/TriAlign_tb.sv:239-260)                  as alignment columns
 *
 * Conventions
 *   - Symbols are one byte each, 0..4 = A,T,C,G,N (src/TriAlign_tb.sv:42-46).
 *     Values > 4 -> TSA_EINVAL. Symbols are reduced mod 4 exactly as the 2-bit
 *     PE symbol registers do (src/PE_1cyc.v:63-66), so N aliases A.
 *   - Lengths >= 1. There is no RTL length envelope here (multiples of 8,
 *     LB <= LA <= 512): results outside it follow the recurrence.
 *   - Return 0 (TSA_OK) or a negative TSA_E* code. Functions are thread-safe
 *     and retain no caller pointer. GPU calls other than *_async are
 *     synchronous.
 *   - Every GPU entry point fails with TSA_ENODEV when no HIP device is
 *     present: there is no CPU fallback in this library.
 */
#ifndef TRIALIGN_H
#define TRIALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSA_OK 0
#define TSA_EINVAL (-1)    /* bad pointer, length, symbol or parameter        */
#define TSA_ERANGE (-2)    /* score range cannot be represented exactly       */
#define TSA_ENODEV (-3)    /* no HIP device / device index out of range       */
#define TSA_EDEVICE (-4)   /* HIP runtime error                               */
#define TSA_ENOMEM (-5)    /* device allocation failed / workspace too small  */
#define TSA_EINTERNAL (-6) /* kernel self-check failed                        */

/* Score reported for a triple the device could not score (a lap-kernel
 * hand-off timed out on tsa_score_batch_async): rescore it. Never a valid
 * score -- every valid score fits 16 bits. The synchronous entry points
 * rescore such triples themselves (tsa_fallback_count counts it). */
#define TSA_SCORE_INVALID INT32_MIN

/* Score reported by TSA_KERNEL_CHECKED for a triple whose values may have
 * left the SCORE_BITS range (so the RTL's wrapped result may differ): rescore
 * it with TSA_KERNEL_PLANE. The synchronous entry points do that themselves
 * (tsa_check_fallback_count counts it). */
#define TSA_SCORE_UNCERTIFIED (INT32_MIN + 1)

#define TSA_S3_RTL 0 /* temp_ABC as the RTL evaluates it (src/PE_1cyc.v:162) */
#define TSA_S3_SOP 1 /* sum of the three pair scores                          */

/* Kernel selection for tsa_score_*; TSA_KERNEL_AUTO picks per shape. */
#define TSA_KERNEL_AUTO 0
/* The literal RTL arithmetic (every candidate wrapped at SCORE_BITS) for any
 * parameter set. Its plan by a cost model: the literal lap schedule for a few
 * cubes, the literal helix for batches of LC <= 512, else the anti-diagonal
 * plane sweep (tsa_describe_plan names it). */
#define TSA_KERNEL_PLANE 1
#define TSA_KERNEL_PENCIL 2 /* register-systolic pencil sweep (factored form)    */
/* The pencil lap kernel in int16 with a range monitor, for cubes whose a-priori
 * bound exceeds SCORE_BITS (beyond ~680 per side with the RTL constants) but
 * whose values may well stay inside it: the factored form is exact whenever
 * no value of the literal recurrence wraps, and the monitor proves that per
 * triple (every real cell's best, then the candidate bound of DESIGN.md 1.2)
 * or reports TSA_SCORE_UNCERTIFIED. TSA_KERNEL_AUTO uses it on the
 * synchronous entry points (rescoring uncertified triples with PLANE); the
 * async path only runs it when asked. Single cubes / small batches (the lap
 * schedule) only: TSA_ERANGE otherwise. */
#define TSA_KERNEL_CHECKED 3

typedef struct tsa_params {
  int32_t match;      /* MATCH      (src/PE_1cyc.v:55), default  1 */
  int32_t mismatch;   /* MISMATCH   (src/PE_1cyc.v:56), default -1 */
  int32_t gap_open;   /* GO         (src/PE_1cyc.v:57), default  2 */
  int32_t gap_extend; /* GE         (src/PE_1cyc.v:58), default  1 */
  int32_t s3_mode;    /* TSA_S3_RTL (default) or TSA_S3_SOP          */
  int32_t score_bits; /* 12 = RTL SCORE_BITS wrap (default); 0 = no wrap
                         (int16 range); any of 4..16 is accepted      */
} tsa_params;

/* Fill *p with the RTL's effective constants (1, -1, 2, 1, RTL s3, 12 bits). */
void tsa_default_params(tsa_params *p);

/* Host-side validation of one triple + params (no device work). */
int tsa_validate(const uint8_t *a, int32_t la, const uint8_t *b, int32_t lb,
                 const uint8_t *c, int32_t lc, const tsa_params *p);

/* Score one triple on HIP device `device` (synchronous). Host buffers. */
int tsa_score_gpu(const uint8_t *a, int32_t la, const uint8_t *b, int32_t lb,
                  const uint8_t *c, int32_t lc, const tsa_params *p,
                  int32_t *score, int32_t device);

/* As tsa_score_gpu with an explicit kernel choice and optional final states:
 * final_states (nullable) receives the 7 states {M,Ix,Iy,Iz,Ixy,Iyz,Ixz} of
 * cell (la,lb,lc) -- the 84-bit SRAM word of src/TriAlign_1cyc.v:130,138; a
 * non-null final_states runs the literal kernels (TSA_KERNEL_PLANE). */
int tsa_score_gpu_ex(const uint8_t *a, int32_t la, const uint8_t *b, int32_t lb,
                     const uint8_t *c, int32_t lc, const tsa_params *p,
                     int32_t kernel, int32_t *score, int32_t *final_states,
                     int32_t device);

/* Score n independent triples held back to back in host memory:
 * triple i is seqs[offsets[3i] .. offsets[3i+1]) = A,
 * [offsets[3i+1] .. offsets[3i+2]) = B, [offsets[3i+2] .. offsets[3i+3]) = C.
 * offsets has 3n+1 entries. Triples are sharded over min(n_devices, visible
 * devices) GPUs (n_devices <= 0: all visible), one host thread per device. */
int tsa_score_batch(const uint8_t *seqs, const int64_t *offsets, int32_t n,
                    const tsa_params *p, int32_t *scores, int32_t n_devices);

/* tsa_score_batch over an explicit device list: the batch is cut into
 * min(n_devices, n) contiguous shards, shard s (triples [n*s/ns, n*(s+1)/ns))
 * on devices[s]. A device may be listed more than once ({0,0,0} shards a
 * batch three ways on one GPU): one host thread per distinct device runs its
 * shards one after another. Same replacement of the testbench's one-shot
 * caller (src/TriAlign_tb.sv:279-333) as tsa_score_batch, which is this call
 * with devices {0..n_devices-1}. TSA_ENODEV for a device index out of range. */
int tsa_score_batch_devices(const uint8_t *seqs, const int64_t *offsets, int32_t n,
                            const tsa_params *p, int32_t *scores,
                            const int32_t *devices, int32_t n_devices);

/* Device-resident batch. d_seqs/d_offsets/d_scores are device pointers on the
 * current device; stream is a hipStream_t (NULL = default stream). The
 * workspace must hold tsa_batch_workspace_size() bytes. max_l* bound every
 * triple's lengths. Launches only; no host synchronisation. Validation of
 * symbols is the caller's job on this path (tsa_validate on the host copy).
 * For a few large cubes this path may run the single-cube (lap) schedule --
 * the factored lap kernel, or for TSA_KERNEL_PLANE the literal lap kernel --
 * whose workgroups hand data to each other. The launched grid is one
 * resident round (8 x SX workgroups, at any workgroups per CU); a cube or
 * batch with more laps than resident slots runs up to LAP_MAX_WAVES (4)
 * rounds as each workgroup's loop over its later-round laps, in lap order.
 * Forward progress needs every launched workgroup co-resident, so a
 * concurrent kernel holding CUs of the device can delay some of them; every
 * hand-off wait is bounded, and if one times out the affected triples read
 * TSA_SCORE_INVALID once the stream has synchronised -- check for it on every
 * kernel choice, TSA_KERNEL_PLANE included. */
int tsa_batch_workspace_size(int32_t n, int32_t max_la, int32_t max_lb,
                             int32_t max_lc, const tsa_params *p,
                             int32_t kernel, size_t *bytes);
int tsa_score_batch_async(const uint8_t *d_seqs, const int64_t *d_offsets,
                          int32_t n, int32_t max_la, int32_t max_lb,
                          int32_t max_lc, const tsa_params *p, int32_t kernel,
                          int32_t *d_scores, void *d_workspace,
                          size_t workspace_bytes, void *stream);

/* tsa_score_batch_async on 2-bit packed sequences: d_packed holds symbol i of
 * the batch buffer at bits [2(i%4)+1 : 2(i%4)] of byte i/4 (tsa_pack2);
 * offsets count symbols, as above. The RTL keeps symbols in 2-bit registers
 * (src/PE_1cyc.v:63-66: N = 4 scores as A), so packing loses nothing; the
 * input is a quarter of the bytes. Same kernels, workspace and semantics. */
int tsa_score_batch_async_p2(const uint8_t *d_packed, const int64_t *d_offsets,
                             int32_t n, int32_t max_la, int32_t max_lb,
                             int32_t max_lc, const tsa_params *p, int32_t kernel,
                             int32_t *d_scores, void *d_workspace,
                             size_t workspace_bytes, void *stream);
/* Pack n symbols (0..4) four to a byte for tsa_score_batch_async_p2; out must
 * hold (n + 3) / 4 bytes. TSA_EINVAL on a symbol above 4. Host only. */
int tsa_pack2(const uint8_t *syms, int64_t n, uint8_t *out);

/* Score ONE triple with its cube split over several GPUs (synchronous): the
 * reference's slicing of the (y,z) plane into pencils chained through face
 * SRAMs (src/TriAlign_1cyc.v:78-98,127-140, pic/Memory.png), distributed --
 * the cube's laps (2*NW rows of y each) are cut into
 * n_devices contiguous runs, part i on devices[i]; the last lap of part i
 * hands its y records to part i+1 by system-scope stores into part i+1's
 * fine-grained workspace over xGMI (peer access is enabled between the listed
 * devices). A device may be listed more than once: its parts then run
 * concurrently on streams of their own when all their workgroups fit on the
 * device at once, else one after another on one stream of that device (a
 * part that waited for CU slots held by a later part could never finish).
 * The concurrent form assumes the device is otherwise idle; if its hand-off
 * times out (another kernel held CU slots) the split is rerun serially and
 * tsa_fallback_count() counts it.
 * The factored arithmetic where
 * it is exact a priori, else the RTL's literal wrapped arithmetic (any
 * parameter set); TSA_ERANGE with fewer laps than n_devices (or no lap
 * schedule). A timed-out hand-off returns TSA_EINTERNAL (never a silent
 * score). wall_us (nullable): host wall time from the first launch to the last
 * part's completion. */
int tsa_score_gpu_multi(const uint8_t *a, int32_t la, const uint8_t *b, int32_t lb,
                        const uint8_t *c, int32_t lc, const tsa_params *p,
                        const int32_t *devices, int32_t n_devices, int32_t *score,
                        double *wall_us);

/* Optimal alignment of one triple (synchronous, HIP device `device`): the
 * path behind the score, as one move per alignment column. This has no RTL
 * counterpart -- the testbench's alignment-output ports are commented out
 * (src/TriAlign_tb.sv:239-260) -- so it is an extension, defined by the same
 * recurrence (src/PE_1cyc.v:164-218) and computed by the literal PLANE
 * arithmetic. moves[k], k < *n_moves, in forward order, is the state of the
 * k-th column, which says which sequences it consumes:
 *   TSA_MOVE_M (a,b,c) _IX (a) _IY (b) _IZ (c) _IXY (a,b) _IYZ (b,c) _IXZ (a,c).
 * start[3] receives the face cell (x0,y0,z0) the path leaves: the zero faces
 * make the start free, so symbols before a[x0], b[y0], c[z0] are not aligned
 * (0-based: the first aligned symbols are a[x0], b[y0], c[z0] as consumed).
 * Ties go to the lowest state index, at the final MAX7 and at every cell.
 * max_moves must be >= la + lb + lc. The pointer cube needs 4*lb*(la+lc-1)*lc
 * bytes of device memory (TSA_ENOMEM when it cannot be allocated). */
#define TSA_MOVE_M 0
#define TSA_MOVE_IX 1
#define TSA_MOVE_IY 2
#define TSA_MOVE_IZ 3
#define TSA_MOVE_IXY 4
#define TSA_MOVE_IYZ 5
#define TSA_MOVE_IXZ 6
int tsa_align_gpu(const uint8_t *a, int32_t la, const uint8_t *b, int32_t lb,
                  const uint8_t *c, int32_t lc, const tsa_params *p, int32_t *score,
                  uint8_t *moves, int32_t max_moves, int32_t *n_moves, int32_t *start,
                  int32_t device);

/* Optimal alignments of a batch of triples (synchronous, HIP device `device`):
 * tsa_align_gpu for n triples in one call. seqs and offsets (3n+1 of them) are
 * laid out as for tsa_score_batch; lengths may differ from triple to triple.
 * moves has the layout of seqs: triple i owns
 *   moves[offsets[3i] - offsets[0] .. offsets[3i+3] - offsets[0])
 * (la+lb+lc bytes), whose first n_moves[i] bytes receive its columns in
 * forward order (TSA_MOVE_*); starts[3i..3i+2] is the face cell its path
 * leaves and scores[i] its score. Per triple the result is that of
 * tsa_align_gpu: literal wrapped arithmetic for every parameter set, lowest
 * state index on ties, free start at the zero faces. Thread-safe; retains no
 * caller pointer. Validation comes before any device work: TSA_EINVAL (or
 * tsa_validate's code) for null pointers, n < 0, non-monotone offsets, bad
 * symbols or parameters; TSA_OK for n == 0; TSA_ENODEV with no HIP device
 * (there is no CPU fallback).
 * A triple whose (y,z) planes fit one workgroup (lb*lc <= 4096 and
 * 32*(lb+1)*(lc+1) + lb + lc bytes within the 160 KiB of LDS; 64 x 64 fits,
 * LA is unbounded) is swept by the resident kernel, one launch for all such
 * triples of a chunk; the others run the plane sweep, one launch per plane for
 * all of them (override align_mode). When a chunk holds at least 256 triples
 * that do not fit, or under align_mode = tiled for any number of them, they
 * are swept by the tiled resident kernel instead: one workgroup per triple
 * sweeps the (y,z) plane in balanced tiles of at most 64 x 48 (or the override
 * align_tile), one after another, and hands the last row and the last column
 * of a tile to its neighbours through a face workspace in device memory
 * (32*la*(lc+1) + 32*la*TY bytes per triple, TY the tile's rows); one more
 * launch per chunk, results identical (tsa_describe_align_plan names the
 * path). The pointer cubes cost 4*lb*(la+lc-1)*lc
 * bytes per triple: the batch is processed in chunks of consecutive triples
 * whose cubes fit a budget -- half of the device memory free at the call, or
 * the override align_tb_bytes -- and a triple whose own cube exceeds the
 * budget is TSA_ENOMEM, as is a failed device allocation. No RTL counterpart
 * (see tsa_align_gpu). */
int tsa_align_batch(const uint8_t *seqs, const int64_t *offsets, int32_t n,
                    const tsa_params *p, int32_t *scores, uint8_t *moves,
                    int32_t *n_moves, int32_t *starts, int32_t device);

/* tsa_align_batch for cubes whose pointer cube exceeds the budget: the same
 * signature, validation, error codes, thread safety and results, move for
 * move, with the plan mode strip unless the override align_mode is set (a set
 * override holds, as everywhere). Triples that fit one workgroup stay with the
 * resident kernel and a whole cube. Every other triple takes the strip path: a
 * strip is one tile row of the tiled kernel, TY rows of y with all of z and x
 * (the same tiles, caps and align_tile override; nty strips). A forward launch
 * sweeps strips 0 .. nty-2 without pointers and keeps the last row of each,
 * which is all the strip above depends on; then launch j = 0, 1, .. sweeps
 * strip nty-1-j of every triple again with pointers into a cube of one strip,
 * and a walk launch follows them until the path leaves the strip or ends --
 * the strips above a path's end are not swept. Per strip triple the need is
 *   4*TY*(la+lc-1)*lc + 16*((nty-1)*la*(lc+1) + 2*la*TY)  bytes
 * (strip cube + kept faces, both counted against the budget; the full cube
 * for a resident triple), about 1/nty of the cube for at most twice the cell
 * work. A chunk holds consecutive triples whose needs fit the budget, and
 * TSA_ENOMEM is returned only when one triple's own need exceeds it. A chunk
 * queues [resident] + [forward, if a strip triple has nty >= 2] + max nty
 * counted launches (tsa_kernel_launch_count). */
int tsa_align_batch_lowmem(const uint8_t *seqs, const int64_t *offsets, int32_t n,
                           const tsa_params *p, int32_t *scores, uint8_t *moves,
                           int32_t *n_moves, int32_t *starts, int32_t device);

/* tsa_align_batch with the larger triples on the grid path: the same
 * signature, validation, error codes, thread safety and results, move for
 * move, with the plan mode grid unless the override align_mode is set (a set
 * override holds, as under tsa_align_batch_lowmem). Triples that fit one
 * workgroup stay with the resident kernel and a whole cube. Every other triple
 * is cut into the tiled kernel's tiles (the same caps and align_tile override;
 * nty x ntz tiles of TY x TZ), and the last row and the last column of every
 * tile are kept: nty-1 y faces [la][lc+1] and ntz-1 z faces [la][lb]. Forward
 * launch d = 0 .. nty+ntz-3 sweeps the tiles with ty + tz = d without pointers,
 * one workgroup per tile -- tiles of one diagonal are independent, and stream
 * order is all that orders the launches. Backward launch j = 0, 1, .. then
 * sweeps again, with pointers into a cube of one tile, only the tile the
 * triple's walker stands in, and of it only x up to the walker's x; a walk
 * launch follows the pointers until the path leaves the tile -- through a y
 * seam, a z seam or the corner -- or ends. A path visits at most nty+ntz-1
 * tiles. Per grid triple the need is
 *   4*TY*(la+TZ-1)*TZ + 16*((nty-1)*la*(lc+1) + (ntz-1)*la*lb)  bytes
 * (tile cube + kept faces, both counted against the budget; the full cube for
 * a resident triple). A chunk holds consecutive triples whose needs fit the
 * budget, and TSA_ENOMEM is returned only when one triple's own need exceeds
 * it. A chunk queues [resident] + max (nty+ntz-2) forward + max (nty+ntz-1)
 * backward counted launches (tsa_kernel_launch_count), the maxima over its
 * grid triples. */
int tsa_align_batch_grid(const uint8_t *seqs, const int64_t *offsets, int32_t n,
                         const tsa_params *p, int32_t *scores, uint8_t *moves,
                         int32_t *n_moves, int32_t *starts, int32_t device);

/* End-free traceback: tsa_align_batch with a choice of where the path may end.
 * The zero faces make the start of every alignment free; the reference takes
 * FINAL_MAX at the corner (LA,LB,LC) alone (src/TriAlign_1cyc.v:141-142), so
 * the entry points above all end there. end_mode selects the cells that may
 * end the path:
 *   TSA_END_CORNER  the cell (la,lb,lc): tsa_align_batch's result
 *   TSA_END_FACE    real cells with x == la or y == lb or z == lc, where one
 *                   sequence is used up (overlap alignment)
 *   TSA_END_ANY     every real cell 1 <= x <= la, 1 <= y <= lb, 1 <= z <= lc
 *                   (the best-scoring triple of prefixes)
 * The end cell (x1,y1,z1) is the candidate whose MAX7 over its 7 states -- the
 * literal wrapped values, compared as the final MAX7 compares them -- is
 * largest; ties between cells go to the smallest x, then the smallest y, then
 * the smallest z, ties between states to the lowest state index. The recurrence
 * is causal, so that MAX7 is the score of the prefixes a[0..x1), b[0..y1),
 * c[0..z1) and the path is their alignment, move for move. scores[i] is that
 * MAX7, ends[3i..3i+2] = (x1,y1,z1); the path is walked from there, through
 * the same pointer words, to the zero face it leaves, and starts, moves and
 * n_moves (always >= 1) are as tsa_align_batch's: the alignment covers
 * a[x0..x1), b[y0..y1), c[z0..z1), and the symbols beyond the end are no more
 * aligned than those before the start.
 *
 * Layouts, validation order, error codes, thread safety, chunking under the
 * pointer-cube budget and align_tb_bytes are tsa_align_batch's; also
 * TSA_EINVAL for a null ends or an end_mode outside 0..2, before any device
 * work. TSA_END_CORNER runs tsa_align_batch's own path, under every plan and
 * override, and fills ends with the lengths. Under TSA_END_FACE and
 * TSA_END_ANY a triple that fits one workgroup takes the resident kernel and
 * every other one the tiled resident kernel, whatever their number (as under
 * tsa_align_batch_async; tsa_describe_align_plan under align_mode = tiled
 * describes the plan); align_tile holds, and a set align_mode of plane, strip
 * or grid returns TSA_EINVAL. Both kernels search the end cell as they sweep,
 * so capacity, tile geometry and budget needs are tsa_align_batch's, and a
 * chunk queues its counted launches under align_mode = tiled:
 * [resident] + [tiled].
 *
 * Not covered: the strip and grid paths, the plane sweep, tsa_align_gpu. A
 * free end on the grid path, for cubes whose pointers do not fit the budget,
 * is tsa_align_batch_grid_ends below; the device-resident form of both is
 * tsa_align_batch_ends_async. The end-free score without a path is
 * tsa_score_batch_ends below; the prefixes it returns can be aligned on
 * every traceback path. */
#define TSA_END_CORNER 0
#define TSA_END_FACE 1
#define TSA_END_ANY 2
int tsa_align_batch_ends(const uint8_t *seqs, const int64_t *offsets, int32_t n,
                         const tsa_params *p, int32_t end_mode, int32_t *scores,
                         uint8_t *moves, int32_t *n_moves, int32_t *starts,
                         int32_t *ends, int32_t device);

/* tsa_align_batch_ends with the larger triples on the grid path of
 * tsa_align_batch_grid: the same signature and the same results for every
 * triple, parameter set and end_mode, move for move. end_mode, scores, ends,
 * starts, moves and n_moves, the tie rule, layouts, validation order, error
 * codes (TSA_EINVAL for a null ends or an end_mode outside 0..2 included) and
 * thread safety are tsa_align_batch_ends's. The plan, the tile geometry,
 * align_tile, align_tb_bytes, chunking, TSA_ENOMEM and the per-triple need,
 *   4*TY*(la+TZ-1)*TZ + 16*((nty-1)*la*(lc+1) + (ntz-1)*la*lb)  bytes,
 * are tsa_align_batch_grid's: the end search takes nothing from the budget (8
 * bytes per tile are allocated beside it).
 *
 * TSA_END_CORNER runs tsa_align_batch_grid's own path under every override and
 * fills ends with the lengths. Under TSA_END_FACE and TSA_END_ANY, with
 * align_mode unset or grid, a triple that fits one workgroup takes the resident
 * kernel with its end search, as under tsa_align_batch_ends, and every other
 * one the grid path: the forward launches sweep every tile, the last one
 * included (d = 0 .. nty+ntz-2), each tile keeps the best end key of its
 * cells, the largest of a triple's keys names the end cell, and the backward
 * launches start from the tile of that cell, of which they sweep x <= x1. A set
 * align_mode of resident or tiled holds, and the call is tsa_align_batch_ends;
 * plane or strip returns TSA_EINVAL before any device work.
 *
 * A chunk queues [resident] + max (nty+ntz-1) forward + max (nty+ntz-1)
 * backward counted launches (tsa_kernel_launch_count), the maxima over its grid
 * triples: one forward launch more than tsa_align_batch_grid. The host does not
 * know the end tile without a synchronisation, so the backward count is the
 * worst case, whatever tile the path ends in; a workgroup whose triple's path
 * has ended leaves before its first barrier.
 *
 * Not covered: the strip path, the plane sweep and tsa_align_gpu. The
 * device-resident form is tsa_align_batch_ends_async
 * (TSA_ALIGN_PATH_GRID). */
int tsa_align_batch_grid_ends(const uint8_t *seqs, const int64_t *offsets, int32_t n,
                              const tsa_params *p, int32_t end_mode, int32_t *scores,
                              uint8_t *moves, int32_t *n_moves, int32_t *starts,
                              int32_t *ends, int32_t device);

/* End-free scores without a path: scores[i] and ends[3i..3i+2] exactly as
 * tsa_align_batch_ends defines them (the same candidates per end_mode, the
 * same MAX7, the same tie rule; no state index), computed by the factored
 * helix scorer as it sweeps, with no memory per cell. The recurrence is
 * causal, so the free-end alignment is the corner alignment of the prefixes
 * a[0..x1), b[0..y1), c[0..z1): screen a batch here, then trace back only the
 * hits with any traceback entry point (tsa_align_batch, _grid, _async ...),
 * or trace the batch back with its free end, without leaving the device, by
 * tsa_align_batch_ends_async.
 *
 * Layouts, validation order and thread safety are tsa_score_batch's and
 * tsa_score_batch_async's (on the async call the symbols are the caller's job,
 * and it only queues work). Errors, in this order and before any device work:
 * TSA_EINVAL for a null pointer (ends included), bad offsets, symbols or
 * parameters, or an end_mode outside 0..2; TSA_OK for n == 0; TSA_ERANGE for a
 * request the plan below does not admit; TSA_ENODEV with no HIP device or a
 * device index out of range. There is no CPU fallback. The synchronous call
 * runs chunks of at most 65535 triples whose workspace stays under the cap of
 * tsa_score_batch, one launch each.
 *
 * TSA_END_CORNER runs tsa_score_batch's own plan (TSA_KERNEL_AUTO; on the
 * async call tsa_score_batch_async's, with tsa_batch_workspace_size's
 * workspace) and fills ends with the lengths. Under TSA_END_FACE and
 * TSA_END_ANY the plan is always the helix with one triple per workgroup --
 * never the lap schedule, never two triples per wave (pencil_two is ignored) --
 * and a request is admitted exactly when tsa_score_batch would score
 * (max_la, max_lb, max_lc) with the factored form in f16-class arithmetic
 * (plain f16, V-space float or V-space integer patterns, as the score plan
 * picks), max_lc <= 256 and max_lb <= 2048 (the end search's key holds the row
 * in 8 bits of laps). The int16 form, literal-only parameter sets
 * (gap_open < gap_extend), pencil_arith = i16 and larger cubes are TSA_ERANGE;
 * a set pencil_mode other than helix is TSA_EINVAL. The workspace is the helix
 * ring of that geometry (tsa_score_ends_workspace_size; it may hold anything
 * on entry); tsa_kernel_launch_count rises by one per helix launch.
 * tsa_describe_score_ends_plan returns the same codes on any host; its text is
 * the helix plan's with " ends=face" or " ends=any" in place of the estimate,
 * and tsa_describe_plan's (synchronous, TSA_KERNEL_AUTO) for the corner.
 *
 * Not covered by these four: the literal helix (tsa_score_batch_ends_ex below
 * is the end-free score where only the literal arithmetic is exact), the lap
 * kernels, cubes with max_lc > 256, and more than one device per call. */
int tsa_score_batch_ends(const uint8_t *seqs, const int64_t *offsets, int32_t n,
                         const tsa_params *p, int32_t end_mode, int32_t *scores,
                         int32_t *ends /* 3n */, int32_t device);
int tsa_score_ends_workspace_size(int32_t n, int32_t max_la, int32_t max_lb,
                                  int32_t max_lc, const tsa_params *p,
                                  int32_t end_mode, size_t *bytes);
int tsa_score_batch_ends_async(const uint8_t *d_seqs, const int64_t *d_offsets,
                               int32_t n, int32_t max_la, int32_t max_lb,
                               int32_t max_lc, const tsa_params *p,
                               int32_t end_mode, int32_t *d_scores,
                               int32_t *d_ends, void *d_workspace,
                               size_t workspace_bytes, void *stream);
int tsa_describe_score_ends_plan(int32_t n, int32_t max_la, int32_t max_lb,
                                 int32_t max_lc, const tsa_params *p,
                                 int32_t end_mode, char *buf, size_t len);

/* The same four with a kernel choice, as tsa_score_gpu_ex is to tsa_score_gpu:
 * the end-free screen in the RTL's literal wrapped arithmetic, so that it
 * returns tsa_align_batch_ends's score and end cell for every parameter set --
 * gap_open < gap_extend, cubes whose a-priori bound leaves the f16 range, and
 * any score_bits, where the words really wrap -- without a pointer cube.
 *
 *   TSA_KERNEL_PENCIL   the call above in every respect: codes, plan text,
 *                       workspace.
 *   TSA_KERNEL_PLANE    the literal helix end search (literal_kernel END): the
 *                       literal helix with one triple per workgroup -- never
 *                       the literal lap, never the plane sweep -- folding the
 *                       MAX7 of every real cell's seven states as it sweeps.
 *                       Admitted for any parameter set with max_la <= 4095,
 *                       max_lb <= 4096 and max_lc <= 256 (and an LDS that
 *                       holds the tables); TSA_ERANGE otherwise. max_lc <= 256
 *                       because only the M = 1 and M = 2 kernels exist: with
 *                       the fold the M = 4 kernel (257..512) does not fit the
 *                       register file without scratch. score_bits = 0 runs in
 *                       16-bit words and is TSA_ERANGE where the unwrapped
 *                       range leaves int16 (as everywhere).
 *   TSA_KERNEL_AUTO     the factored helix where the call above admits the
 *                       request, else the literal end search where that admits
 *                       it, else TSA_ERANGE.
 *   TSA_KERNEL_CHECKED  TSA_ERANGE (no checked end search).
 * Anything outside 0..3 is TSA_EINVAL, checked next to end_mode; the rest of
 * the validation order is the call's above, all before any device work.
 *
 * TSA_END_CORNER fills ends with the lengths and runs the score plan of that
 * kernel (tsa_score_batch_async's on the async call, with
 * tsa_batch_workspace_size's workspace for that kernel). The literal end
 * search's workspace is the literal ring of the geometry
 * (tsa_score_ends_workspace_size_ex; it may hold anything on entry), its plan
 * text "plane literal-helix M=<m> P=<p> ends=face|any" and the overrides;
 * tsa_kernel_launch_count rises by one per launch, one launch per chunk of at
 * most 65535 triples.
 *
 * Overrides: under PLANE and AUTO pencil_mode = literal forces the literal end
 * search; under AUTO pencil_mode = helix forces the factored one (TSA_ERANGE
 * where it does not admit the request); any other set pencil_mode is
 * TSA_EINVAL.
 *
 * Not covered: an end search on the literal lap or the plane sweep, cubes with
 * max_lc > 256, and more than one device per call. */
int tsa_score_batch_ends_ex(const uint8_t *seqs, const int64_t *offsets, int32_t n,
                            const tsa_params *p, int32_t end_mode, int32_t kernel,
                            int32_t *scores, int32_t *ends /* 3n */, int32_t device);
int tsa_score_ends_workspace_size_ex(int32_t n, int32_t max_la, int32_t max_lb,
                                     int32_t max_lc, const tsa_params *p,
                                     int32_t end_mode, int32_t kernel, size_t *bytes);
int tsa_score_batch_ends_async_ex(const uint8_t *d_seqs, const int64_t *d_offsets,
                                  int32_t n, int32_t max_la, int32_t max_lb,
                                  int32_t max_lc, const tsa_params *p,
                                  int32_t end_mode, int32_t kernel, int32_t *d_scores,
                                  int32_t *d_ends, void *d_workspace,
                                  size_t workspace_bytes, void *stream);
int tsa_describe_score_ends_plan_ex(int32_t n, int32_t max_la, int32_t max_lb,
                                    int32_t max_lc, const tsa_params *p,
                                    int32_t end_mode, int32_t kernel, char *buf,
                                    size_t len);

/* The same four on the lap schedule, for the cubes the two families above
 * refuse (max_lc > 256: one 512^3 or 1024^3 cube, a handful of large ones):
 * scores[i] and ends[3i..3i+2] exactly as tsa_align_batch_ends defines them,
 * found by the checked int16 lap kernel as it sweeps (lap_ends_kernel: every
 * register half keeps one key {best : ~(x - 1)} of its candidate cells, a
 * reduction kernel takes the triple's largest), with no memory per cell.
 * Layouts, validation order and thread safety are tsa_score_batch_ends'.
 * Errors, in this order and before any device work: TSA_EINVAL for a null
 * pointer (ends included), bad offsets, symbols or parameters, an end_mode
 * outside 0..2, or (under face and any) a set pencil_mode other than lap;
 * TSA_OK for n == 0; TSA_ERANGE for a request the admission below refuses;
 * TSA_ENODEV.
 *
 * TSA_END_CORNER runs tsa_score_batch's own plan (on the async call
 * tsa_score_batch_async's under TSA_KERNEL_CHECKED, with
 * tsa_batch_workspace_size's workspace for that kernel) and fills ends with
 * the lengths. Under TSA_END_FACE and TSA_END_ANY a request is admitted exactly
 * when TSA_KERNEL_CHECKED admits (max_la, max_lb, max_lc) -- the factored form
 * is exact a priori, or its int16 carrier holds the a-priori bound and only the
 * SCORE_BITS wrap has to be ruled out by the certificate -- and a lap plan
 * exists for (n, maxima) among the end search's geometries (M = 1, 2 pairs per
 * lane, NW = 4, 8 waves; chunked as the score plans are). The call never runs
 * the helix, the literal forms or the split over devices; lap_m, lap_nw,
 * lap_chunk and lap_spin_limit hold. Where the form is exact a priori nothing
 * is certified; where it is only checkable the checked kernel's rule runs, and
 * a certified triple's result is exact because no value of its cube wraps.
 *
 * A triple that is not certified reads TSA_SCORE_UNCERTIFIED on the async call,
 * one whose launch had a hand-off time out TSA_SCORE_INVALID, both with ends
 * 0, 0, 0. The synchronous call rescores such triples through
 * tsa_align_batch_grid_ends' host path (literal arithmetic, any size) and
 * discards the moves: tsa_check_fallback_count rises by one per uncertified
 * triple, tsa_fallback_count once per chunk that timed out.
 *
 * The workspace is the checked lap workspace of the geometry plus the key
 * slots, 8 bytes per compute wave of every logical workgroup
 * (tsa_score_ends_workspace_size_lap, host-only; it may hold anything on
 * entry). tsa_kernel_launch_count rises by one per lap launch. The plan text is
 * the checked lap plan's with " ends=face" or " ends=any" in place of the
 * estimate (" checked" where certification runs), and tsa_describe_plan's
 * (synchronous, TSA_KERNEL_AUTO) for the corner.
 *
 * Not covered: an end search on the literal lap, on a cube split over devices,
 * the M = 4 geometries, and more than one device per call. */
int tsa_score_batch_ends_lap(const uint8_t *seqs, const int64_t *offsets, int32_t n,
                             const tsa_params *p, int32_t end_mode, int32_t *scores,
                             int32_t *ends /* 3n */, int32_t device);
int tsa_score_ends_workspace_size_lap(int32_t n, int32_t max_la, int32_t max_lb,
                                      int32_t max_lc, const tsa_params *p,
                                      int32_t end_mode, size_t *bytes);
int tsa_score_batch_ends_async_lap(const uint8_t *d_seqs, const int64_t *d_offsets,
                                   int32_t n, int32_t max_la, int32_t max_lb,
                                   int32_t max_lc, const tsa_params *p,
                                   int32_t end_mode, int32_t *d_scores,
                                   int32_t *d_ends, void *d_workspace,
                                   size_t workspace_bytes, void *stream);
int tsa_describe_score_ends_plan_lap(int32_t n, int32_t max_la, int32_t max_lb,
                                     int32_t max_lc, const tsa_params *p,
                                     int32_t end_mode, char *buf, size_t len);

/* Device-resident traceback: tsa_align_batch on sequences that are already in
 * device memory, with results that stay there. d_* are device pointers on the
 * current device, stream is a hipStream_t (NULL = default stream). h_offsets
 * is a host copy of the same 3n+1 offsets: the call reads it for validation
 * and planning and never after it returns; the device reads d_offsets. That the
 * two agree is the caller's job, as is the validation of symbols (tsa_validate
 * on the host copy), exactly as for tsa_score_batch_async.
 * Outputs are laid out as tsa_align_batch's: triple i owns
 *   d_moves[h_offsets[3i] - h_offsets[0] .. h_offsets[3i+3] - h_offsets[0]),
 * whose first d_n_moves[i] bytes receive its columns in forward order; the
 * bytes of the slot beyond them are not written. d_starts[3i..3i+2] and
 * d_scores[i] as in tsa_align_batch. d_n_moves[i] == 0 is never a valid result:
 * it flags a triple whose walk came out of range (what the synchronous entry
 * points report as TSA_EINTERNAL). Results equal tsa_align_batch's for every
 * triple and parameter set, move for move: literal wrapped arithmetic, lowest
 * state index on ties, free start.
 * The call only queues work: no device allocation, no copy to or from host
 * memory, no query of free memory, no stream of its own and no
 * synchronisation (the metadata of a chunk is built by a kernel from d_offsets,
 * since a copy from pageable host memory would wait for the stream).
 * Thread-safe; two calls in flight need two workspaces.
 * Triples that fit one workgroup run the resident kernel with a whole cube;
 * the others take `path`: TSA_ALIGN_PATH_TILED the tiled resident kernel,
 * whatever their number (the plane sweep is not available here: it costs
 * la+lb+lc launches per chunk and its workspace is not additive per triple;
 * tsa_describe_align_plan under align_mode = tiled describes the plan),
 * TSA_ALIGN_PATH_STRIP the strip path of tsa_align_batch_lowmem,
 * TSA_ALIGN_PATH_GRID the grid path of tsa_align_batch_grid. Overrides:
 * align_tile holds as everywhere; a set align_mode of tiled, strip or grid
 * replaces `path` (a set override holds), align_mode = resident or plane makes
 * tsa_align_workspace_size and tsa_align_batch_async return TSA_EINVAL;
 * align_tb_bytes, when set, caps the budget of a chunk from above.
 * The workspace (256-byte aligned) holds a fixed part sized for the whole call
 * -- the packed sequences and moves, the metadata of the chunks, the results
 * and the walker records of strip or grid triples, each region 256-byte
 * aligned -- then the face buffers and the pointer cubes of one chunk. The
 * budget of a chunk is workspace_bytes minus the fixed part, and a triple's
 * need against it is: resident, the cube (4*lb*(la+lc-1)*lc bytes); tiled, the
 * cube plus its face workspace (32*la*(lc+1) + 32*la*TY bytes); strip and grid,
 * the needs stated at tsa_align_batch_lowmem and tsa_align_batch_grid. Chunks
 * are consecutive triples whose needs fit the budget together, at most 65535,
 * and a chunk queues the counted launches (tsa_kernel_launch_count) of the
 * synchronous entry point of its path; the helper kernels that build the
 * metadata, pack the sequences and scatter the results, and the walks, are not
 * counted. tsa_align_workspace_size (host-only, no device needed, validation
 * as below) prices that plan: min_bytes = the fixed part + the largest need of
 * a triple, the smallest workspace the call succeeds with; full_bytes = the
 * size from which the batch takes the fewest chunks possible. Any size in
 * between works, with more chunks.
 * Validation comes before any device work: TSA_EINVAL for null pointers,
 * n < 0, non-monotone h_offsets or a length below 1, bad parameters, an unknown
 * path, an override value that is not valid or a workspace that is not
 * 256-byte aligned; TSA_OK for n == 0; TSA_ENODEV with no HIP device;
 * TSA_ENOMEM when workspace_bytes < min_bytes, with nothing queued. No RTL
 * counterpart (see tsa_align_gpu). */
#define TSA_ALIGN_PATH_TILED 0 /* larger triples: tiled resident kernel, whole cube */
#define TSA_ALIGN_PATH_STRIP 1 /* ... the strip path of tsa_align_batch_lowmem       */
#define TSA_ALIGN_PATH_GRID 2  /* ... the grid path of tsa_align_batch_grid          */
int tsa_align_workspace_size(const int64_t *h_offsets, int32_t n, const tsa_params *p,
                             int32_t path, size_t *min_bytes, size_t *full_bytes);
int tsa_align_batch_async(const uint8_t *d_seqs, const int64_t *d_offsets,
                          const int64_t *h_offsets, int32_t n, const tsa_params *p,
                          int32_t path, int32_t *d_scores, uint8_t *d_moves,
                          int32_t *d_n_moves, int32_t *d_starts,
                          void *d_workspace, size_t workspace_bytes, void *stream);

/* Device-resident end-free traceback: tsa_align_batch_ends and
 * tsa_align_batch_grid_ends under tsa_align_batch_async's calling convention.
 * Two contracts joined:
 *  - the results -- d_scores, d_ends (3n: the end cell x1,y1,z1), d_starts,
 *    d_moves, d_n_moves -- are tsa_align_batch_ends's (tsa_align_batch_grid_ends's
 *    under TSA_ALIGN_PATH_GRID; the two agree) for every triple, parameter set
 *    and end_mode, move for move: the same candidates, MAX7 over the literal
 *    wrapped states, ties to the smallest x, then y, then z, then the lowest
 *    state;
 *  - pointers, h_offsets, stream, output layout, thread safety and the promise
 *    to only queue launches -- no allocation, no host copy, no free-memory
 *    query, no synchronisation -- are tsa_align_batch_async's. Only the first
 *    d_n_moves[i] bytes of a moves slot are written; d_n_moves[i] == 0 flags a
 *    triple whose walk came out of range or whose end key names no cell, and
 *    d_ends of such a triple is unspecified.
 * TSA_END_CORNER runs tsa_align_batch_async's own plan for `path` (tiled, strip
 * or grid) and fills d_ends with the lengths, on the device. Under
 * TSA_END_FACE and TSA_END_ANY a triple that fits one workgroup takes the
 * resident kernel with its end search; every other one takes the tiled
 * resident kernel's under TSA_ALIGN_PATH_TILED and the grid path's under
 * TSA_ALIGN_PATH_GRID (forward over every tile with a key slot per tile, the
 * end records, then backward from the end tile, x <= x1);
 * TSA_ALIGN_PATH_STRIP is TSA_EINVAL. Overrides: align_tile holds; a set
 * align_mode of tiled or grid replaces `path`; strip, resident or plane is
 * TSA_EINVAL; align_tb_bytes caps a chunk's budget from above. A chunk raises
 * tsa_kernel_launch_count as the synchronous entry point of its path does:
 * [resident] + [tiled], or [resident] + max (nty+ntz-1) forward +
 * max (nty+ntz-1) backward on the grid path; helper kernels and walks are not
 * counted.
 * The workspace is tsa_align_batch_async's; the end records lie on a region the
 * end search leaves unused. On the grid path with a free end the fixed part has
 * two more 256-byte-rounded regions: n int64 slot offsets and 8 bytes per tile
 * of every over-capacity triple of the call (S = the sum of nty*ntz, whatever
 * the chunks; they may hold anything on entry). So tsa_align_ends_workspace_size
 * equals tsa_align_workspace_size under TSA_END_CORNER and under
 * TSA_ALIGN_PATH_TILED, and exceeds it by up256(8n) + up256(8S) under
 * TSA_ALIGN_PATH_GRID with a free end. It is host-only.
 * Validation, all before any device work and in this order: TSA_EINVAL for a
 * null pointer (d_ends included), a workspace that is not 256-byte aligned, an
 * end_mode outside 0..2, whatever tsa_align_batch_async rejects, and the path
 * and override combinations above; TSA_OK for n == 0; TSA_ENODEV; TSA_ENOMEM
 * when workspace_bytes < min_bytes, with nothing queued.
 * Not covered: a free end on the strip path, the plane sweep or tsa_align_gpu,
 * and more than one device per call. */
int tsa_align_ends_workspace_size(const int64_t *h_offsets, int32_t n, const tsa_params *p,
                                  int32_t path, int32_t end_mode,
                                  size_t *min_bytes, size_t *full_bytes);
int tsa_align_batch_ends_async(const uint8_t *d_seqs, const int64_t *d_offsets,
                               const int64_t *h_offsets, int32_t n, const tsa_params *p,
                               int32_t path, int32_t end_mode, int32_t *d_scores,
                               uint8_t *d_moves, int32_t *d_n_moves, int32_t *d_starts,
                               int32_t *d_ends /* 3n */, void *d_workspace,
                               size_t workspace_bytes, void *stream);

/* The three gapped rows of n alignments, on the device (queues one launch on
 * stream, no synchronisation, no workspace). d_seqs and d_offsets as above;
 * d_moves, d_n_moves and d_starts in tsa_align_batch's layout, from
 * tsa_align_batch_async, tsa_align_batch_ends_async or uploaded from any of the synchronous entry points.
 * d_rows has three times the layout of d_moves: triple i, of len_i = la+lb+lc
 * symbols, owns 3*len_i bytes at d_rows + 3*(offsets[3i] - offsets[0]), row r
 * (0 = A, 1 = B, 2 = C) at + r*len_i. The first d_n_moves[i] bytes of each row
 * receive one code per alignment column, "ATCGN-"[code]: the symbol the column
 * consumes from that sequence (0..4 as stored, N stays 4) or TSA_ROW_GAP. The
 * bytes beyond them are not written, and nothing is when d_n_moves[i] is 0.
 * Moves that do not belong to these sequences give unspecified rows but no
 * access outside the buffers. TSA_EINVAL for a null pointer or n < 0, TSA_OK
 * for n == 0, TSA_ENODEV with no HIP device. */
#define TSA_ROW_GAP 5
int tsa_align_rows_async(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n,
                         const uint8_t *d_moves, const int32_t *d_n_moves,
                         const int32_t *d_starts, uint8_t *d_rows, void *stream);

/* Which path tsa_align_batch takes for a group (one chunk) of n triples of
 * these lengths under the current overrides, as a short text that begins with
 * "resident", "tiled", "strip", "grid" or "plane"; for tiled it carries the tile and
 * the tile grid, such as "tiled tile=64x43 tiles=4x6 lds=91632 faces=5259264"
 * (lds: dynamic LDS of the workgroup, faces: bytes of the triple's face
 * workspace), for strip also the bytes of the strip cube, such as
 * "strip tile=7x7 tiles=3x3 lds=2080 cube=16240 faces=8960", for grid the
 * bytes of the tile cube and of the kept faces, such as
 * "grid tile=7x7 tiles=3x3 lds=2080 cube=3136 faces=13120".
 * It is built from the functions the dispatch uses. Host-only, no device
 * needed. TSA_EINVAL for a null or empty buffer, n or a length below 1, bad
 * parameters, or an align_mode / align_tile value that is not valid. */
int tsa_describe_align_plan(int32_t n, int32_t la, int32_t lb, int32_t lc,
                            const tsa_params *p, char *buf, size_t len);

/* Which kernel, arithmetic and schedule a batch of these sizes would run, as a
 * short text such as "pencil lap f16 rtl M=1 NW=16 laps=16 tiles=1 waves=1"
 * or "plane" (sync = 1: the synchronous tsa_score_batch path, which may stream
 * the lap kernel). Host-only, no device needed. A diagnostic with no reference
 * counterpart (the RTL has one fixed datapath). */
int tsa_describe_plan(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc,
                      const tsa_params *p, int32_t kernel, int32_t sync, char *buf,
                      size_t len);

/* Lap-kernel hand-offs that timed out on the synchronous entry points since
 * the library was loaded; each was rescored without the lap schedule (the
 * helix, or for the literal arithmetic the literal helix / plane sweep) and
 * logged to stderr. 0 in a healthy run. */
int64_t tsa_fallback_count(void);

/* Triples the checked kernel could not certify on the synchronous entry points
 * since the library was loaded; each was rescored in the literal arithmetic
 * (TSA_KERNEL_PLANE's plan). */
int64_t tsa_check_fallback_count(void);

/* Kernel launches with dynamic LDS (helix, lap, literal helix; the resident
 * and the tiled resident traceback kernel of tsa_align_batch, each one per
 * chunk that has triples for it; the forward and the strip launches of the
 * strip path; the forward launches, one per diagonal of the tile grid, and the
 * backward launches of the grid path) the library has queued
 * since it was loaded: a call that reuses an error left over from an earlier
 * HIP call must still launch its kernel exactly once (tests). The plane sweep
 * and the traceback walks are not counted. */
int64_t tsa_kernel_launch_count(void);

/* Number of visible HIP devices (0 when none), or a negative code. */
int tsa_device_count(void);

/* Short description of a return code. */
const char *tsa_strerror(int rc);

/* Library build id, "trialign-mi355x gfx950 src=<hash>": the first 16 hex
 * digits of a SHA-256 over the library's sources (csrc .hip and .h files and
 * this header; srchash.py), so a run names the sources its binary came from.
 * While plan overrides are set, " overrides=<tsa_get_overrides text>" follows
 * (the string is then the calling thread's, valid until its next call). */
const char *tsa_version(void);

/* Plan overrides: force a kernel, arithmetic or geometry the planner would
 * not pick on its own (parity tests of every schedule, same-process A/B
 * timing). The library reads no environment variable to plan; these named
 * values, set explicitly, are the only way to steer it, and while any is set
 * tsa_describe_plan and tsa_version say so. Process-wide and thread-safe;
 * scores stay exact under every override (only speed and the plan change).
 *   pencil_mode     helix | lap | plane | literal | litlap
 *   pencil_arith    i16 | f16       (factored arithmetic: int16, f16 w/o V-space)
 *                   f16vf | f16vi   (the V-space helix: f16vf keeps the float
 *                   cell; f16vi asks for the cell on integer bit patterns and
 *                   is TSA_EINVAL for a launch that cannot run it)
 *   pencil_two      0 | 1           (two triples per helix wave for LC <= 64)
 *   lap_m, lap_nw   lap tile pairs per lane (1,2,4) / compute waves (4,8)
 *   lap_vs          0 | 1           (the lap kernel's V-space cell)
 *   lap_chunk       triples per lap launch of a chunked batch
 *   lap_spin_limit  polls before a lap hand-off times out (0: at once)
 *   lap_trace       path of a per-workgroup timestamp CSV (tools/lap_trace.py)
 *   split_serial    0 | 1           (tsa_score_gpu_multi parts one by one)
 *   align_mode      resident | plane | tiled | strip | grid (tsa_align_batch: resident
 *                   still sends a triple that does not fit a workgroup to the
 *                   plane sweep; tiled sends it to the tiled resident kernel,
 *                   strip to the strip path of tsa_align_batch_lowmem, grid
 *                   to the grid path of tsa_align_batch_grid, and under any
 *                   of the three no triple takes the plane sweep)
 *   align_tb_bytes  pointer-cube budget of a tsa_align_batch chunk, in bytes
 *   align_tile      TYxTZ, e.g. 5x7: caps the tile edges of the tiled kernel;
 *                   under align_mode = tiled, strip or grid every triple larger than
 *                   the tile is tiled, even one that would fit a workgroup. A malformed
 *                   value, an edge below 1 or a tile over the tiled kernel's
 *                   capacity (the resident capacity, and TY*TZ <= 3072) makes tsa_align_batch and tsa_describe_align_plan return
 *                   TSA_EINVAL
 * value NULL clears `name`; name NULL clears every override. TSA_EINVAL for an
 * unknown name or a value longer than 255 bytes. The reference has no
 * counterpart: its datapath parameters are fixed at build (src/PE_1cyc.v:55-61). */
int tsa_set_override(const char *name, const char *value);

/* The active overrides as "name=value,name=value" in name order ("" when none),
 * NUL-terminated into buf (truncated to len - 1). Returns the full length. */
int tsa_get_overrides(char *buf, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* TRIALIGN_H */
