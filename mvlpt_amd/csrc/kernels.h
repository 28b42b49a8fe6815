// Launcher declarations for the hand-written gfx950 kernels (gemm.hip, norm.hip, attention.hip, glue.hip, ...).
// Every launcher only enqueues on the given stream; no hidden synchronisation.
#pragma once
#include "common.h"

struct MvlptOptimHyper;      // include/mvlpt_hip.h
struct MvlptOptimSeg;

namespace mvlpt {

// ---------------------------------------------------------------- streams with a compute-unit partition (engine.hip)
// Compute units the kernels of `s` can run on: the partition size for a stream made by mvlpt_stream_create_cus, the whole
// device otherwise.  Persistent / grid-stride launchers size their grids from it.
int stream_cus(hipStream_t s);
// The same without the grid cap of mvlpt_stream_set_cu_cap.  A launcher that chooses between two kernels whose results differ in the
// last bit (the persistent attention forward against one workgroup per head) chooses by THIS count and sizes the grid by stream_cus:
// a cap then changes how many workgroups run, never which arithmetic.
int stream_cus_nocap(hipStream_t s);

// ---------------------------------------------------------------- row map
// The leading `seq` positions of sequences that are saved at a pitch of `pitch` rows: compact row r belongs to saved row
// (r / seq) * pitch + r % seq.  seq == 0: the identity.  The one statement of the map: every launcher that reads a saved tensor from
// compact rows (GemmArgs::aux_rows, LnBwdArgs::x_rows, ActArgs::u_rows, launch_copy_rows) carries this struct and calls row().
struct RowMap {
  int seq = 0, pitch = 0;
  __host__ __device__ size_t row(int r) const { return seq > 0 ? (size_t)(r / seq) * pitch + r % seq : (size_t)r; }
};
// When a map is legal for `rows` compact rows: whole sequences, pitch >= seq, and the saved rows below 2^31.  Each launcher adds
// its own conditions to this one.
inline bool row_map_ok(RowMap m, int rows) {
  if (m.seq == 0) return true;
  return m.seq > 0 && m.pitch >= m.seq && rows % m.seq == 0 && (int64_t)(rows / m.seq) * m.pitch <= INT32_MAX;
}

// ---------------------------------------------------------------- GEMM  C = A * Bt^T (+ epilogue)
enum GemmEpi {
  EPI_STORE16 = 0,  // out16 = acc (+bias)
  EPI_GELU = 1,     // u = acc+bias ; out2 (optional, 16-bit) = u ; out16 = QuickGELU(u)
  EPI_RESID32 = 2,  // out32 = acc + bias + resid32          (fp32 residual stream, may alias out)
  EPI_GELUBWD = 3,  // out16 = acc * QuickGELU'(aux16)       (aux = saved pre-activation u)
  EPI_STORE32 = 4,  // out32 = acc (+bias)
  // split-precision outputs: a 16-bit pair (hi = round16(v), lo = round16(v - hi)) stored as ONE row of 2N elements
  // [hi(0..N) | lo(0..N)], i.e. directly the `a_split` A operand of the next GEMM
  EPI_GELU_SPLIT = 5,     // u = acc+bias ; out2 (optional, 16-bit [M,N]) = u ; out [M,2N] = split(QuickGELU(u))
  EPI_GELUBWD_SPLIT = 6,  // out [M,2N] = split(acc * QuickGELU'(aux16))
  EPI_STORE_SPLIT = 7,    // out [M,2N] = split(acc (+bias))
  // EPI_RESID32 that also PRODUCES the input of the LayerNorm behind it in folded form (GemmArgs::ln_*, "LayerNorm folding")
  EPI_RESID32_LN = 8,
  // internal: EPI_STORE16 / EPI_GELU / EPI_STORE_SPLIT / EPI_GELU_SPLIT with the consumer side of the folding compiled in
  // (launch_gemm selects them when GemmArgs::fold_part is set; callers pass the plain values)
  EPI_STORE16_FOLD = 9, EPI_GELU_FOLD = 10, EPI_STORE_SPLIT_FOLD = 11, EPI_GELU_SPLIT_FOLD = 12,
  // EPI_RESID32_LN on the PACKED residual stream (fp16, single operands; GemmArgs::rp_*): the stream is read and written as
  // hi (16-bit, [M,N]) + lo (one byte, [M,N]) — common.h respk_* — and the hi plane IS the consumer's A operand (the LayerNorm's
  // gamma is folded into the consumer's weight instead of into the activation): no fp32 stream, no separate 16-bit copy
  EPI_RESIDP_LN = 13,
};
constexpr int epi_base(int epi) {
  return epi == EPI_STORE16_FOLD ? EPI_STORE16 : epi == EPI_GELU_FOLD ? EPI_GELU : epi == EPI_STORE_SPLIT_FOLD ? EPI_STORE_SPLIT
         : epi == EPI_GELU_SPLIT_FOLD ? EPI_GELU_SPLIT : epi;
}
constexpr bool epi_folds(int epi) { return epi >= EPI_STORE16_FOLD && epi <= EPI_GELU_SPLIT_FOLD; }
constexpr bool epi_ln_producer(int epi) { return epi == EPI_RESID32_LN || epi == EPI_RESIDP_LN; }
struct GemmArgs {
  const void* A = nullptr;       // [M,K] 16-bit
  const void* Bt = nullptr;      // [N,K] 16-bit
  int M = 0, N = 0, K = 0;
  const float* bias = nullptr;   // [N] or null
  const void* aux = nullptr;     // [M,N] 16-bit (EPI_GELUBWD)
  const float* resid = nullptr;  // [M,N] fp32   (EPI_RESID32)
  void* out = nullptr;           // [M,N]
  void* out2 = nullptr;          // [M,N] 16-bit, optional (EPI_GELU)
  // Split-precision A operand: A is [M, 2K] = [A_hi | A_lo] (16-bit pair, A ~ A_hi + A_lo to ~22 bits) and the
  // product is A_hi*Bt^T + A_lo*Bt^T in the same fp32 accumulators: the K loop runs over 2K with the Bt K-index wrapping.
  // The frozen weights are exactly representable in 16 bits (they are stored so, clip/model.py:371-392), so the product
  // then carries the activations at ~fp32 precision.  Costs twice the MFMA work.
  // a_split == 2 (mixed pair): A is [M, 2K] 16-bit slots per row (same pitch) holding [A_hi (K x 16 bit) | A_lo8 (K bytes) | unused],
  // A_lo8 = e5m2(A_lo * 2^Lo8<T>::EXP) (common.h), and Bt rows hold [W16 (K x 16 bit) | W8 (K bytes)] with pitch ldb >= 3K/2
  // elements, W8 = e4m3(W * 2^w8_exp): the product is A_hi*W16^T on v_mfma_f32_16x16x32 plus A_lo8*W8^T on
  // v_mfma_scale_f32_16x16x128_f8f6f4 (twice the rate, the e8m0 scale operands undo the two exponents) in the same
  // accumulators: 1.5x the matrix time of a single-operand GEMM instead of 2x; the operand is carried to ~2^-14 (fp16) / ~2^-11
  // (bf16) of its value (e5m2 residual x e4m3 weight copy; tests/test_hip_mixed_pair.py asserts these per-element bounds).
  // K % 128 == 0.
  int a_split = 0;
  int ldb = 0;         // Bt row pitch in 16-bit elements (0: K)
  int w8_exp = 0;      // a_split == 2: exponent of the weight's fp8 plane
  int out_lo8 = 0;     // EPI_GELU_SPLIT / EPI_GELUBWD_SPLIT: store the pair as [hi | lo8] (mixed pair) instead of [hi | lo]
  // Row pitches in 16-bit elements (0: dense).  lda: rows of A (dense: K, or 2K with a_split); ldo: rows of `out` for the pair-producing
  // epilogues 5 / 6 / 7 (dense: 2N).  A pitch that is a multiple of 4 KiB puts the same K-stage of every row on the same memory
  // channels (M = 7 700, K = 2048 pair rows of 8 KiB: 56 vs 36 us next to K = 1920 / 2176, profiles/r04_pitch_probe.txt): the engine
  // pads such rows by 128 bytes.
  int lda = 0, ldo = 0;
  int xcd_order = 0;   // set by the one-tile-per-workgroup launcher (gemm_pc_kernel): XCD-aware tile order
  // EPI_GELUBWD / EPI_GELUBWD_SPLIT: output row m reads aux row aux_rows.row(m) (sequences of at least 3 rows)
  RowMap aux_rows;
  // ---- LayerNorm folding: LN(x) W^T = rstd_r * ((x * gamma) W^T)[r,n] - rstd_r * mean_r * (W gamma)[n] + (W beta)[n], so the
  // GEMM in front of a LayerNorm hands the un-normalised row to the GEMM behind it and the LayerNorm pass (one read of the fp32
  // residual stream + one 16-bit write per LayerNorm) disappears.  No atomics, no extra launch: every output tile owns its slots.
  // Producer (EPI_RESID32_LN): besides out32 = acc + bias + resid32 the epilogue stores ln_x16 = round16(out32 * ln_gamma) — the A
  // operand of the consumer, format ln_split: 0 [M,N], 1 hi|lo pair [M,2N], 2 mixed pair (same pitch) — and, per row and block j of
  // 128 output columns (independent of the tile geometry), the partial sums {sum out32, sum out32^2} at ln_part[(row * ln_ntp + j) * 2].
  const float* ln_gamma = nullptr;
  void* ln_x16 = nullptr;
  int ln_split = 0;
  float* ln_part = nullptr;
  int ln_ntp = 0;               // slots per row (>= N / 128, even)
  // Consumer (EPI_STORE16 / EPI_GELU / EPI_STORE_SPLIT / EPI_GELU_SPLIT with fold_part != null): A holds round16(x * gamma);
  // mean / rstd of row r are rebuilt from its fold_nt partials (summed in slot order: deterministic) and the epilogue computes
  // rstd_r * acc - rstd_r * mean_r * fold_colsum[n] + bias[n], with fold_colsum = W gamma and bias = b + W beta precomputed
  // (frozen weights).  K is the length of the normalised rows.  The partials of a tile's rows ride along with its last K-stage
  // (LDS-DMA into a 16 KiB region behind the ring), so the epilogue reads them from LDS.
  const float* fold_part = nullptr;
  const float* fold_colsum = nullptr;
  int fold_ntp = 0, fold_nt = 0;
  // ---- packed residual stream (EPI_RESIDP_LN): the stream in front of the GEMM is rp_hi_in [M,N] fp16 + rp_lo_in [M,N] bytes,
  // the updated stream goes to `out` [M,N] fp16 (hi) + rp_lo_out [M,N] bytes; ln_part / ln_ntp as for EPI_RESID32_LN (the
  // statistics are those of the fp32 value before it is packed).  In place (in == out) is allowed: a tile reads what it rewrites.
  const void* rp_hi_in = nullptr;
  const uint8_t* rp_lo_in = nullptr;
  uint8_t* rp_lo_out = nullptr;
#ifdef MVLPT_GEMM_TRACE
  long long* trace = nullptr;   // debug builds only: per-wave (point id << 56 | s_memtime) records of workgroup 0
#endif
};
// N-tile width the launcher picks for this problem on this stream
int gemm_tile_n(int dtype, int epi, const GemmArgs& g, hipStream_t s);
// Which of the seven GEMM kernels the launcher picks for a problem on a stream (gemm.hip launch_one; kernel-level tests assert it,
// so that a moved routing threshold cannot silently move their coverage).  Values are part of the C ABI (mvlpt_op_gemm_route).
enum GemmFamily {
  GEMM_FAM_BT_128x128_R2 = 1,  // gemm_bt_kernel 128x128, 2-deep ring, two workgroups per compute unit
  GEMM_FAM_BT_128x128_R4 = 2,  // gemm_bt_kernel 128x128, 4-deep ring
  GEMM_FAM_BT_256x128_R3 = 3,  // gemm_bt_kernel 256x128, 3-deep ring
  GEMM_FAM_BT_256x256_R2 = 4,  // gemm_bt_kernel 256x256, 2-deep ring
  GEMM_FAM_PHASED = 5,         // gemm_bt_phased_kernel (256x128, 3-deep ring)
  GEMM_FAM_PC = 6,             // gemm_pc_kernel (128x128, 4-deep ring, one tile per workgroup)
  GEMM_FAM_PCP = 7,            // gemm_pcp_kernel (256x128, 3-deep ring, persistent with movers)
};
struct GemmRoute { int family = 0, tile_m = 0, tile_n = 0, ring = 0; };
// (reads M, N, K, a_split and fold_ntp of `g`; `folded`: a folded consumer, i.e. a launch with fold_part set)
hipError_t gemm_route(int dtype, int epi, const GemmArgs& g, bool folded, hipStream_t s, GemmRoute* r);
// ev_start/ev_stop (optional): recorded by the dispatch itself (hipExtLaunchKernelGGL): kernel-exact timing with no
// extra marker packets on the stream.
hipError_t launch_gemm(int dtype, int epi, const GemmArgs& g, hipStream_t s, hipEvent_t ev_start = nullptr,
                       hipEvent_t ev_stop = nullptr);

// fp32 GEMM on the f32-input MFMA (exact f32 products, v_mfma_f32_16x16x4_f32) for the two tiny projections
// next to the logits (CLS / EOT rows only): C[M,N] = alpha * A[M,K] * Bt[N,K]^T.  K % 16 == 0, N % 4 == 0.
hipError_t launch_sgemm_bt(const float* A, const float* Bt, float* C, int M, int N, int K, const float* alpha_dev, hipStream_t s);

// ---------------------------------------------------------------- LayerNorm (fp32 statistics)
// Input row r is read at  x + in_row(r) * d  with in_row(r) = row_idx ? row_idx[r] : r * row_mul.
struct LnFwdArgs {
  const float* x = nullptr; const int32_t* row_idx = nullptr; int row_mul = 1;
  const float* gamma = nullptr; const float* beta = nullptr;
  void* y = nullptr;   // [rows,d] contiguous, 16-bit (out_dtype = compute dtype) or fp32 (out_dtype = DT_F32)
  int rows = 0, d = 0;
  int split = 0;    // 16-bit outputs only: y is [rows, 2d] = [hi | lo] (split-precision A operand, see GemmArgs::a_split);
                    // 2: same pitch, [hi | lo8 bytes | unused] (mixed pair)
};
hipError_t launch_ln_fwd(int out_dtype, const LnFwdArgs& a, hipStream_t s);

struct LnBwdArgs {
  const void* dy = nullptr;        // [rows,d] contiguous, 16-bit (dy_dtype = compute dtype) or fp32 (dy_dtype = DT_F32)
  int dy_dtype = DT_F32;
  const float* x = nullptr; const int32_t* row_idx = nullptr; int row_mul = 1;   // LN input rows (same mapping as forward)
  const float* gamma = nullptr;
  const float* resid = nullptr;    // fp32, same row mapping as x, or null:  out32 = resid + dx
  float* out32 = nullptr;          // fp32, same row mapping as x (may alias resid)
  void* out16 = nullptr;           // optional 16-bit copy, same row mapping
  int rows = 0, d = 0;
  int split = 0;         // out16 is [*, 2d] = [hi | lo]; 2: [hi | lo8 bytes | unused] (mixed pair)
  // a map (row_idx null, row_mul 1): x alone is read at row x_rows.row(r); dy, resid and the outputs stay at row r
  RowMap x_rows;
};
hipError_t launch_ln_bwd(int dtype, const LnBwdArgs& a, hipStream_t s);
// The kernel both launchers use for `rows` x `d` on stream `s`: stream = 0 one wave per row (ln_*_kernel), 1 grid-stride
// (ln_*_stream_kernel<.., nv>); grid = its workgroups of 4 waves.  Part of the C ABI (mvlpt_op_layernorm_route).
struct LnRoute { int stream, nv, grid; };
LnRoute ln_route(int rows, int d, hipStream_t s);

// ---------------------------------------------------------------- attention (head_dim 64)
// fmt 0 (single 16-bit operands, attention.hip; L <= 256 resident, longer sequences streamed):
//   qkv: [N*L, 3*d] 16-bit, token = n*L + i, columns [q | k | v], head h at h*64 inside each third; out [N*L, d].
// fmt 1 / 2 (split-precision attention, attention32.hip, any L) — the mode of the towers that carry a gradient: every operand is a
//   16-bit hi|lo pair [rows, 2*cols] (hi = round16(x), lo = round16(x - hi)), products keep hi*hi + hi*lo + lo*hi on the 16-bit MFMA
//   (fp32 accumulation); the outputs are pairs again: directly the `a_split` A operand of the next GEMM.
//   qkv: [N*L, 6d] 16-bit: [hi(q|k|v) | lo(q|k|v)], head h at h*64 inside each d-wide block; out [N*L, 2d]: [hi(d) | lo(d)].
//   fmt 2 (mixed pair): `out` rows are [hi(d) | lo8 (d bytes) | unused], the out-projection's A operand.
struct AttnArgs {
  const void* qkv = nullptr; void* out = nullptr; float* lse = nullptr /*[N*H*L] or null*/;
  int N = 0, L = 0, H = 0; int causal = 0;
  int q_rows = 0;   // > 0: only queries 0..q_rows-1 of every sequence are computed (last layer: only CLS is consumed)
  int flags = 0;    // experiment bits: 1 = non-temporal K/V staging, 2 = non-temporal output stores (fmt 0; set by launch_attn_fwd)
  // Shared prefix (the short causal kernels: causal, L <= 80, q_rows == 0, 2 P <= L).  prefix = P > 0: positions 0 .. P-1 are the same
  // rows in all N sequences and every tensor holds N + 1 "slots" of L - P rows: slot 0 = the prefix in its first P rows, slot n + 1 =
  // positions P .. L-1 of sequence n (lse: [slot, H, L - P]).  Sequence n reads position p < P from slot 0 and writes only its
  // queries >= P; one more workgroup row (pairs: blockIdx.y == N; single operands: workgroups (N, h)) is the prefix itself, length P;
  // it also writes zeros into the other rows of slot 0 of out / lse (never read by the attention: the row-wise kernels behind it
  // then meet finite, deterministic values).
  int prefix = 0;
  // Operand format: 0 single 16-bit, 1 hi|lo pair, 2 mixed pair — the encoding of TowerState::xs, GemmArgs::a_split, LnFwdArgs::split
  int fmt = 0;
#ifdef MVLPT_ATTN_TRACE
  long long* trace = nullptr;   // debug builds only (tools/attn_trace.py): (point id << 56 | s_memtime) records of one workgroup
#endif
};
// Routes on a.fmt.  ea / eb (optional): start / stop events of the kernel's own dispatch (hipExtLaunchKernelGGL), for
// mvlpt_profile_* — the resident single-operand kernels only
hipError_t launch_attn_fwd(int dtype, const AttnArgs& a, hipStream_t s, hipEvent_t ea = nullptr, hipEvent_t eb = nullptr);
struct AttnBwdArgs {
  const void* qkv = nullptr; const void* out = nullptr; const void* dout = nullptr /*[N*L, d]; pairs: [N*L, 2d]*/;
  const float* lse = nullptr;
  float* delta = nullptr /*[N*H*L] scratch*/; void* dqkv = nullptr /*[N*L, 3d]; pairs: [N*L, 6d] = [hi(3d) | lo(3d)]*/;
  int N = 0, L = 0, H = 0; int causal = 0;
  // Ls > L: the saved tensors (qkv, out, lse) hold sequences of Ls positions and only the leading L carry a gradient: dout, delta and
  // dqkv are [N*L, .] and positions >= L are neither staged nor computed (causal only: no row < L reads a key or query >= L; pairs:
  // the short causal kernel, L <= 80, only).  0: L
  int Ls = 0;
  // Shared prefix (AttnArgs::prefix; the short causal kernels only, 2 P <= L).  The saved tensors hold N + 1 slots of Ls - P rows,
  // dout / dqkv N + 1 slots of L - P rows, delta [N + 1, H, L - P].  Sequence n takes dO of its positions < P as zero, stores dQ / dK /
  // dV of its positions >= P and writes dK / dV of the prefix keys as fp32 into kv_part [N + 1, P, 2d] (row: dK (d) | dV (d));
  // workgroup row N is the prefix's own backward from slot 0 of dout (dQ into slot 0 of dqkv, dK / dV into kv_part[N]).  One more
  // launch then writes dK / dV of slot 0: kv_part[N] + part_mul * sum_n kv_part[n] (a fixed order, no atomics; single operands in
  // the order of attn32t_prefix_reduce_kernel), and zeroes the unused rows P .. L-P-1 of slot 0.
  int prefix = 0; float* kv_part = nullptr; float part_mul = 1.f;
  // Operand format, as AttnArgs::fmt.  2: `out` rows are [hi | lo8] (read for delta) and dqkv rows are written as
  // [hi(3d) | lo8 (3d bytes) | unused]
  int fmt = 0;
#ifdef MVLPT_ATTN_TRACE
  long long* trace = nullptr;   // debug builds only (tools/attn_trace.py bwd): records of one workgroup of attn32r_bwd_kernel
#endif
};
hipError_t launch_attn_bwd(int dtype, const AttnBwdArgs& a, hipStream_t s);      // routes on a.fmt
int attn_max_len();
// backward when only query 0 of every sequence carries a gradient: o_cls / do_cls are compact [N, H*64] rows
hipError_t launch_attn_bwd_cls(int dtype, const void* qkv, const void* o_cls, const void* do_cls, const float* lse, void* dqkv,
                               int N, int L, int H, hipStream_t s);
// streaming variants (attention_stream.hip): any L, 32 KiB LDS ring; launch_attn_* picks between the two families
hipError_t launch_attn_fwd_stream(int dtype, const AttnArgs& a, hipStream_t s);
hipError_t launch_attn_bwd_stream(int dtype, const AttnBwdArgs& a, hipStream_t s);
// heads wider than 64 (attention_wide.hip): head h at h*head_width inside each third, head_width in {80, 96, 112, 128}, any L, non-causal
// (causal != 0 -> hipErrorInvalidValue), forward only; only rows 0..q_rows-1 of every sequence are written when q_rows > 0
bool attn_wide_supported(int head_width);
hipError_t launch_attn_fwd_wide(int dtype, const AttnArgs& a, int head_width, hipStream_t s);

// ---------------------------------------------------------------- input pipeline (preprocess.hip)
// same layout as MvlptImageDesc (include/mvlpt_hip.h)
struct PpDesc {
  int64_t offset;                            // byte offset of pixel (0,0) of this image in the packed uint8 HWC source
  int32_t height, width;
  int32_t crop_top, crop_left, crop_h, crop_w;
  int32_t resize_h, resize_w;                // size the crop box is resampled to
  int32_t out_top, out_left;                 // window of the resized image that is produced (CenterCrop); 0,0 for training
  int32_t flip, reserved;
};
hipError_t launch_preprocess(const uint8_t* src, const PpDesc* descs_dev, int B, int max_crop_h, int ks_max, int out_h, int out_w,
                             int32_t* tables, size_t table_stride, uint8_t* tmp, size_t tmp_stride, const float* mean,
                             const float* stdv, void* out, int out_dtype, uint8_t* out_u8, hipStream_t s);
// same layout as MvlptAugmentDesc (include/mvlpt_hip.h)
constexpr int PP_AUG_MAX_OPS = 4, PP_AUG_MAX_HOLES = 4;
enum { PP_OP_BRIGHTNESS = 0, PP_OP_CONTRAST = 1, PP_OP_SATURATION = 2, PP_OP_HUE = 3 };
struct PpAug {
  int32_t n_ops, ops[PP_AUG_MAX_OPS];        // colour operations in the order they are applied
  float factor[3];                           // brightness, contrast, saturation
  int32_t hue_shift, grayscale, n_holes;
  int32_t hole[PP_AUG_MAX_HOLES][4];         // top, left, height, width inside the output window
};
// the FILL form of the three kernels above (a window index outside the resized image produces 0), the vertical pass writing only the
// flipped 8-bit window `win` [B,out_h,out_w,3], then the colour chain / grayscale / holes in place on it and ToTensor / Normalize
hipError_t launch_preprocess_aug(const uint8_t* src, const PpDesc* descs_dev, const PpAug* augs_dev, int B, int max_crop_h, int ks_max,
                                 int out_h, int out_w, int32_t* tables, size_t table_stride, uint8_t* tmp, size_t tmp_stride, uint8_t* win,
                                 const float* mean, const float* stdv, void* out, int out_dtype, hipStream_t s);

// ---------------------------------------------------------------- JPEG decode (jpeg.hip; the structures are in jpeg_core.h)
namespace jpeg { struct ImgDesc; struct PlaneDesc; struct Tables; struct Seg; }
// entropy stage of n_images images: coefficient blocks (int16 [64], natural order; `coefs` zeroed by the caller) and status[d.index]
hipError_t launch_jpeg_entropy(const uint8_t* src, const jpeg::ImgDesc* descs_dev, const jpeg::Tables* tables_dev, const jpeg::Seg* segs_dev,
                               int n_images, int16_t* coefs, int32_t* status, hipStream_t s);
// dequantise + IDCT of every component plane (max_blocks: the largest n_blocks among them)
hipError_t launch_jpeg_idct(const jpeg::PlaneDesc* planes_dev, int n_planes, int max_blocks, const jpeg::Tables* tables_dev,
                            const int16_t* coefs, uint8_t* planes, hipStream_t s);
hipError_t launch_jpeg_idct_one(const jpeg::PlaneDesc& p, const uint8_t* quant_dev, const int16_t* coefs, uint8_t* plane, hipStream_t s);
// upsample + colour into dst + d.dst_off, packed HWC RGB (max_groups: the largest ceil(width / 4) * height)
hipError_t launch_jpeg_colour(const jpeg::ImgDesc* descs_dev, int n_images, long long max_groups, const uint8_t* planes, uint8_t* dst,
                              hipStream_t s);
hipError_t launch_jpeg_colour_one(const jpeg::ImgDesc& d, const uint8_t* planes, uint8_t* dst, hipStream_t s);

// ---------------------------------------------------------------- glue
hipError_t launch_cast_f32_to16(int dtype, const float* in, void* out, size_t n, const float* scale_dev, hipStream_t s);
// fp32 [rows,d] (* scale_dev[0]) -> 16-bit pair [rows, 2d] = [hi | lo]
// (lo8 = 1: [hi | lo8 bytes | unused], the mixed pair)
hipError_t launch_cast_f32_split(int dtype, const float* in, void* out, size_t rows, int d, const float* scale_dev, hipStream_t s, int lo8 = 0);
hipError_t launch_cast_any_to_f32(int in_dtype, const void* in, float* out, size_t n, hipStream_t s);
// W [rows, cols] (fp32) -> out16 [rows, ld_out] zero padded (cols <= ld_out)
hipError_t launch_pack_weight(int dtype, const float* w, void* out, int rows, int cols, int ld_out, hipStream_t s);
// fp8 plane of a packed weight: out8[r, c] = e4m3(W[r, c] * scale_dev[0]) (transposed = 1: out8[c, r]), zero padded to `cols_out`
// bytes per row; `out8` points at the plane inside the 16-bit rows, pitch_bytes apart
hipError_t launch_pack_weight8(const float* w, uint8_t* out8, int rows, int cols, int transposed, int cols_out, size_t pitch_bytes,
                               const float* scale_dev, hipStream_t s);
// W [rows, cols] (fp32) -> out16 [cols, rows] (transposed)
hipError_t launch_pack_weight_t(int dtype, const float* w, void* out, int rows, int cols, hipStream_t s, int ld_out = 0);
// image [B,3,R,R] (fp32 / f16 / bf16) -> patches16 [B*g*g, Kp], column order (c,ky,kx), zero padded to Kp
hipError_t launch_patchify(int dtype, const void* image, int image_dtype, void* out, int B, int R, int P, int Kp, hipStream_t s);
// the kernel launch_patchify uses: 0 patchify_kernel (scalar), 1 patchify_vec_kernel, 2 patchify16_kernel (mvlpt_op_patchify_route)
int patchify_route(int dtype, int image_dtype, int R, int P);
// tokens: row0 = LN(cls + pos0); rows 1..n = vpt; rest = LN(patch + pos)   (trainers/mvlpt.py:56-62)
hipError_t launch_assemble_tokens(const float* patch_emb, const float* cls, const float* pos, const float* g, const float* b,
                                  const float* vpt, int n_vpt, float* x, int B, int G2, int d, hipStream_t s,
                                  const float* vmask = nullptr /* [B, n_vpt, d] dropout mask of the prompt rows, or null */);
// the same rows (no prompts) straight into the packed residual stream (hi [B*(1+G2), d] fp16, lo bytes) + the rows' {sum, sum of
// squares} in slot 0 of `part` [rows][ntp][2]
hipError_t launch_assemble_tokens_packed(const float* patch_emb, const float* cls, const float* pos, const float* g, const float* b,
                                         void* hi, uint8_t* lo, float* part, int ntp, int B, int G2, int d, hipStream_t s);
// x[b, 1+j, :] = rows[j, :]   (deep prompt overwrite, trainers/mvlpt.py:78-82)
hipError_t launch_overwrite_rows(const float* rows, int n, float* x, int B, int L, int d, hipStream_t s, const float* vmask = nullptr);
// prompts (forward_coop + positional embedding, trainers/mvlpt.py:439-515, 107/112)
hipError_t launch_assemble_prompts(const float* prefix, const float* suffix, const float* ctx, int ctx_per_class, int n_ctx,
                                   const int32_t* layout, const float* pos, float* x, int C, int L, int d, hipStream_t s,
                                   int shared_prefix = 0);
// shared_prefix = P > 0: the three tables / tokens in the shared-prefix layout (AttnArgs::prefix; glue.hip): x as C + 1 slots of
// L - P rows, eot rows in slot c + 1, ctx_pos against gradient slots of Lt rows
hipError_t launch_build_ctx_pos(const int32_t* layout, int32_t* ctx_pos, int C, int L, int n_ctx, hipStream_t s, int shared_prefix = 0, int Lt = 0);
hipError_t launch_eot_rows(const int32_t* eot, int32_t* rows, int C, int L, hipStream_t s, int shared_prefix = 0);
// token ids (clip/model.py encode_text): x [S, L, d] = emb[ids[s, t]] + pos[t]; ids int32 [S, ld], ld >= L, columns 0 .. L-1 read, every one
// of them inside the table (checked on the host by the callers); d % 4 == 0
hipError_t launch_embed_tokens(const float* emb, const float* pos, const int32_t* ids, int ld, float* x, int S, int L, int d, hipStream_t s);
// dst[r] = src[idx[r]] (scatter = 0) or dst[idx[r]] = src[r] (scatter = 1); row_bytes % 16 == 0
// far (a map): idx names rows of the saved tensors and the far side is compact, holding the leading far.seq positions of every
// sequence of far.pitch: the map read backwards.  An idx[r] whose position the far side does not hold is skipped.
hipError_t launch_copy_rows(const void* src, void* dst, const int32_t* idx, int rows, int row_bytes, int scatter, hipStream_t s,
                            RowMap far = RowMap());
// rows of row_bytes (multiple of 16) from src + r*src_pitch to dst + r*dst_pitch
hipError_t launch_copy_rows_strided(const void* src, void* dst, int rows, size_t src_pitch, size_t dst_pitch, int row_bytes, hipStream_t s);
// out[j,:] = inv_scale * sum_b dx[b, row0+j, :]; optionally zero those rows of dx32/dx16 afterwards
hipError_t launch_reduce_prompt_rows(int dtype, float* dx32, void* dx16, int B, int L, int d, int row0, int n, float* out,
                                     const float* scale_dev, int zero_after, hipStream_t s, int split16 = 0, const float* vmask = nullptr);
// dctx (generic) [n,d] = inv_scale * sum_c dx[c, ctx_pos[c,j], :]  or (per class) [C,n,d]
// shared_prefix > 0: dx holds C + 1 slots of L rows and ctx_pos is launch_build_ctx_pos's table for it; the rows of slot 0 are
// multiplied by pre_mul (the power of two the prefix gradient was scaled down by)
hipError_t launch_gather_ctx_grad(const float* dx, const int32_t* ctx_pos, int C, int L, int d, int n_ctx, int per_class,
                                  float* dctx, const float* scale_dev, hipStream_t s, int shared_prefix = 0, float pre_mul = 1.f);
// ranged prompts (one context block of ctx [G, n_ctx, d] per image, trainers/cocoop.py:123-161; under the per-task mask of
// trainers/mvlpt.py:556-581 only the image's own classes): group g owns classes [lo[g], lo[g] + start[g+1] - start[g]); its
// sequences start[g] .. start[g+1] - 1 are those classes in order.  seq_cls / seq_grp int32 [S]: class and group of every sequence;
// lo int32 [G], start int32 [G + 1] (prefix sum, start[G] = S).  The tables are built and checked on the host (engine.hip).
// CoCoOp's grouped tower and head are the case of every range full (s = g*C + c).
hipError_t launch_assemble_prompts_ranged(const float* prefix, const float* suffix, const float* ctx, int n_ctx, const int32_t* layout,
                                          const float* pos, float* x, const int32_t* seq_cls, const int32_t* seq_grp, int S, int L, int d,
                                          hipStream_t s);
hipError_t launch_eot_rows_ranged(const int32_t* eot, int32_t* rows, const int32_t* seq_cls, int S, int L, hipStream_t s);
// dctx (ranged) [G,n,d] = inv_scale * sum_k dx[start[g] + k, ctx_pos[lo[g] + k, j], :]  (ctx_pos per class, [C, n]); zeros for an empty range
hipError_t launch_gather_ctx_grad_ranged(const float* dx, const int32_t* ctx_pos, const int32_t* lo, const int32_t* start, int G, int L,
                                         int d, int n_ctx, float* dctx, const float* scale_dev, hipStream_t s);
// deep text prompts (deep_text.hip): x[c, ctx_pos[c,j], :] = rows[j, :] over x [C,L,d] fp32, rows [n_ctx,d], ctx_pos int32 [C,n_ctx]; d % 4 == 0
hipError_t launch_overwrite_ctx_rows(const float* rows, const int32_t* ctx_pos, float* x, int C, int L, int d, int n_ctx, hipStream_t s);
// out [n_ctx,d] = inv_scale * sum_c dx32[c, ctx_pos[c,j], :] in gather_ctx_grad's fixed order (the same bits), then those rows of dx32 and
// of its 16-bit copy dx16 (may be null; split16 0: [C*L, d], 1: hi|lo pair [C*L, 2d], 2: mixed pair at the same pitch) are zeroed
hipError_t launch_gather_zero_ctx_grad(int dtype, float* dx32, void* dx16, int split16, const int32_t* ctx_pos, int C, int L, int d,
                                       int n_ctx, float* out, const float* scale_dev, hipStream_t s);
// scale_dev[0] = 2^k with amax(|v|)*2^k ~ target ; scale_dev[1] = 1/scale_dev[0]
hipError_t launch_grad_scale(const float* v, size_t n, float target, float* scale_dev, hipStream_t s);
// fused optimizer step over the flat prompt buffers (optim.hip; semantics in include/mvlpt_hip.h, mvlpt_op_optim_step); the
// arguments are checked by the caller (engine.hip)
hipError_t launch_optim_step(const MvlptOptimHyper& h, float* param, const float* grad, float* state1, float* state2, int64_t n,
                             const MvlptOptimSeg* segs_dev, int n_segs, const float* loss_dev, int32_t* skipped_dev, hipStream_t s);
hipError_t launch_zero(void* p, size_t bytes, hipStream_t s);
hipError_t launch_checksum(const void* p, size_t bytes, unsigned long long* out, hipStream_t s);      // debug (mvlpt_debug_checksums)
// LayerNorm folding: colsum[n] = sum_k W16[n,k] gamma[k], bias2[n] = b[n] + sum_k W16[n,k] beta[k]  (W16 [N, ld] packed weight)
hipError_t launch_fold_vectors(int dtype, const void* W16, int ld, const float* gamma, const float* beta, const float* b,
                               float* colsum, float* bias2, int N, int K, hipStream_t s);

// packed residual stream (common.h respk_*, EPI_RESIDP_LN; fp16 only): gamma folded into the consumer's weight
// (Wg = round16(W16 * gamma), colsum = its row sums), fp32 rows -> packed rows (+ LayerNorm-folding partials in slot 0 of ntp,
// or part = null), packed rows r * row_mul -> fp32 rows
hipError_t launch_fold_weight(const void* W16, int ld, const float* gamma, void* Wg16, int ldg, float* colsum, int N, int K, hipStream_t s);
hipError_t launch_respk_pack_rows(const float* x, void* hi, uint8_t* lo, float* part, int ntp, int rows, int d, hipStream_t s);
hipError_t launch_respk_unpack_rows(const void* hi, const uint8_t* lo, int row_mul, float* out, int rows, int d, hipStream_t s);

// ---------------------------------------------------------------- stand-alone MLP activation (activation.hip)
// The towers' activation (values are part of the C ABI: MVLPT_ACT_*).  ACT_QUICKGELU is what the GEMM epilogues EPI_GELU* compute;
// ACT_GELU (nn.GELU, the erf form) runs as its own element-wise pass between the two MLP GEMMs.
enum ActKind { ACT_QUICKGELU = 0, ACT_GELU = 1 };
// A-operand formats of the output (GemmArgs::a_split of the GEMM that reads it): [M, N], hi|lo pair [M, 2N], mixed pair (same pitch)
enum ActFmt { ACT_FMT_SINGLE = 0, ACT_FMT_PAIR = 1, ACT_FMT_MIXED = 2 };
struct ActArgs {
  const float* in = nullptr;      // forward: the pre-activation u; backward: dA; fp32 [M, N], as EPI_STORE32 writes them
  int ldi = 0;                    // row pitch of `in` in floats (0: dense)
  void* out = nullptr;            // act(u) / dA * act'(u) in format fmt
  int fmt = ACT_FMT_SINGLE;
  int ldo = 0;                    // row pitch of `out` in 16-bit elements (0: dense, N or 2N)
  void* u16 = nullptr;            // 16-bit [M, N], dense: forward, optional: the saved pre-activation is written; backward: it is read
  int M = 0, N = 0;               // N % 8 == 0; pitches multiples of 8; every pointer 16-byte aligned
  // backward only: row m reads u16 row u_rows.row(m) (GemmArgs::aux_rows for the stand-alone pass)
  RowMap u_rows;
};
const char* act_check(int dtype, int act, bool bwd, ActArgs& a);      // null when the launch is legal (pitches resolved), else why not
hipError_t launch_act_fwd(int dtype, int act, const ActArgs& a, hipStream_t s);
hipError_t launch_act_bwd(int dtype, int act, const ActArgs& a, hipStream_t s);

// ---------------------------------------------------------------- head: cosine logits + cross-entropy (fp32)
hipError_t launch_normalize_rows(const float* x, float* xn, float* norm, int rows, int d, hipStream_t s);
// prompt ensembling (trainers/zsclip.py:88-96): out [C, e] = normalize(mean_t normalize(feats[t, c])), feats [T, C, e]; fixed summation
// order over t; T == 1 gives the bits of launch_normalize_rows; e <= 1024
hipError_t launch_ensemble_features(const float* feats, float* out, int T, int C, int e, hipStream_t s);
hipError_t launch_logits(const float* imn, const float* txn, float scale, const int32_t* lo, const int32_t* hi,
                         float* logits, int B, int C, int e, hipStream_t s);
hipError_t launch_cross_entropy(const float* logits, const void* labels, int label_kind, int B, int C, float* row_loss,
                                float* loss, float* dlogits, float* ncorrect, hipStream_t s);
hipError_t launch_logits_bwd(const float* dlogits, const float* imn, const float* txn, const float* inorm, const float* tnorm,
                             float scale, const int32_t* lo, const int32_t* hi, float* dimg, float* dtxt,
                             int B, int C, int e, hipStream_t s);
// ranged head: logits[g,c] = scale * imn[g] . txn[start[g] + c - lo[g]] for lo[g] <= c < lo[g] + (start[g+1] - start[g]), 0 elsewhere;
// backward: dtxt [S, e] and / or dimg [G, e] (through the image normalisation); dlogits outside the ranges is not read
hipError_t launch_logits_ranged(const float* imn, const float* txn, float scale, const int32_t* lo, const int32_t* start, float* logits,
                                int G, int C, int e, hipStream_t s);
hipError_t launch_logits_ranged_bwd(const float* dlogits, const float* imn, const float* txn, const float* inorm, const float* tnorm,
                                    float scale, const int32_t* lo, const int32_t* start, const int32_t* seq_grp, float* dimg, float* dtxt,
                                    int G, int S, int C, int e, hipStream_t s);

// ---------------------------------------------------------------- convolutional tower (conv.hip; fp16 only, forward only)
// y [B,Ho,Wo,Cout] = act(conv(x [B,H,W,Cin], w) * scale[c] + shift[c] (+ resid [B,Ho,Wo,Cout])), NHWC fp16, one rounding.
// k in {1, 3}, pad k/2, stride 1 (2 with k = 3 only), Cin % 8 == 0, Cout % 8 == 0; w is the packed [Cout, conv_kp(k, Cin)] weight of
// launch_pack_conv_weight; scale / shift fp32 [Cout], 16-byte aligned.
struct ConvArgs {
  const void* x; const void* w; const float* scale; const float* shift; const void* resid; void* y;
  int B, H, W, Cin, Cout, k, stride, relu;
};
int conv_kp(int k, int cin_pad);                     // packed row length: k*k*cin_pad rounded up to the K-step
const char* conv2d_check(const ConvArgs& a);         // null when the launch is legal, else what is wrong with it
hipError_t launch_conv2d(const ConvArgs& a, hipStream_t s);
// w32 [Cout,Cin,k,k] fp32 -> out [Cout, conv_kp(k, cin_pad)] fp16, tap-major (ky, kx, ci), channels Cin .. cin_pad-1 and the tail zero
hipError_t launch_pack_conv_weight(const float* w32, void* out, int Cout, int Cin, int k, int cin_pad, hipStream_t s);
// BatchNorm with running statistics as an affine map: scale = g / sqrt(var + eps), shift = b - mean * scale
hipError_t launch_bn_affine(const float* g, const float* b, const float* mean, const float* var, float eps, float* scale, float* shift,
                            int C, hipStream_t s);
// AvgPool2d(2) on NHWC fp16 (fp32 sum, one rounding); C % 8 == 0, odd H / W drop their last row / column as torch does
hipError_t launch_avgpool2x2(const void* x, void* y, int B, int H, int W, int C, hipStream_t s);
// image [B,3,R,R] (fp32 / fp16 / bf16) -> [B,R,R,8] fp16, channels 3..7 zero
hipError_t launch_nchw_to_nhwc8(const void* image, int image_dtype, void* out, int B, int R, hipStream_t s);
// AttentionPool2d: tok [B, 1+HW, E] fp16 = [mean over HW (fp32) ; x] + pos [1+HW, E] fp32;  out [B,E] = single-query attention of
// q [B,E] over kv [B,T,2E] = [K | V], heads of 64, fp32 scores and softmax, T <= attnpool_max_tokens()
int attnpool_max_tokens();
hipError_t launch_attnpool_tokens(const void* x, const float* pos, void* tok, int B, int HW, int E, hipStream_t s);
hipError_t launch_attnpool_query(const void* q, const void* kv, void* out, int B, int T, int E, hipStream_t s);

// ---------------------------------------------------------------- nearest table rows (nearest.hip; semantics in include/mvlpt_hip.h)
// Geometry of one call: row tiles of NR_ROWS query rows (grid.y) x vocabulary slices (grid.x), NR_WAVES partial lists of k keys per
// row and slice.  The slice count follows the stream's compute units; the results do not depend on it.  The arguments are checked by
// the caller (engine.hip): 1 <= k <= min(V, 64), d % 4 == 0, row_tiles <= 65535, ws of ws_bytes.
constexpr int NR_ROWS = 8, NR_WAVES = 4;
struct NearestPlan { int row_tiles = 0, slices = 0, tiles_per_slice = 0, parts = 0; size_t ws_bytes = 0; };
NearestPlan nearest_plan(int R, int V, int k, int cus);
hipError_t launch_nearest_rows(const float* q, const float* table, int R, int V, int d, int k, int32_t* idx, float* dist, void* ws,
                               const NearestPlan& p, hipStream_t s);

// ---------------------------------------------------------------- test-time prompt tuning head (tpt.hip; semantics in include/mvlpt_hip.h)
// Workspace layout of one call, a function of (G, V, C, e, k) alone; offsets in floats, every section on a 256-byte boundary: the
// normalised image and text rows, |txt|, the views' softmax statistics (max, log sum), the selection, then logp, a and dz of the
// selected views.  The arguments are checked by the caller (engine.hip).
struct TptPlan { size_t off_imn = 0, off_tn = 0, off_nt = 0, off_m = 0, off_ls = 0, off_sel = 0, off_lp = 0, off_a = 0, off_dz = 0, ws_bytes = 0; };
TptPlan tpt_plan(int G, int V, int C, int e, int k);
hipError_t launch_tpt_head_fwd(const float* img, const float* txt, float scale, int G, int V, int C, int e, int k, float* loss, float* H,
                               int32_t* sel, float* z, void* ws, const TptPlan& p, hipStream_t s);
hipError_t launch_tpt_head_bwd(const float* w, float scale, int G, int V, int C, int e, int k, float* dtxt, void* ws, const TptPlan& p,
                               hipStream_t s);

// ---------------------------------------------------------------- softmax regression (softmax_reg.hip; semantics in include/mvlpt_hip.h)
// Geometry and workspace layout of one call, a function of (N, D, K) alone: the logits / residuals Z [N, ldz] first (all that predict
// needs: predict_bytes), then `slices` partial [K, D] gradients, their column sums, the loss partials of the row blocks and the
// partial statistics of the final reduce.  The arguments are checked by the caller (engine.hip).
constexpr int SR_TILE = 128;
struct SoftmaxRegPlan {
  int ldz = 0, slices = 0, rows_per_slice = 0, row_blocks = 0, fin_blocks = 0;
  size_t off_part = 0, off_colsum = 0, off_lossp = 0, off_bstats = 0, ws_bytes = 0, predict_bytes = 0;
};
SoftmaxRegPlan softmax_reg_plan(int N, int D, int K);
hipError_t launch_softmax_reg_eval(const float* X, const int32_t* y, const float* theta, const float* dir, int N, int D, int K, double l2,
                                   float* grad, double* stats, void* ws, const SoftmaxRegPlan& p, hipStream_t s);
hipError_t launch_softmax_reg_predict(const float* X, const float* theta, int N, int D, int K, int32_t* pred, float* margin, void* ws,
                                      const SoftmaxRegPlan& p, hipStream_t s);

// ---------------------------------------------------------------- Tip-Adapter head (tip.hip; semantics in include/mvlpt_hip.h)
// Workspace layout of one call, a function of the sizes and the mode alone (byte offsets, sections on 256-byte boundaries).
// MVLPT_TIP_TRAIN: the keys' classes, A^T [NK, ldn], R^T [C, ldn], the logits [N, C] (unused when the caller takes them), the loss and
// hit partials of the row blocks.  MVLPT_TIP_SEARCH: clip [C, chunk_rows] and cache [C, nb, chunk_rows] of one row chunk; the chunk is
// a whole number of row blocks of TIP_ROWS.  MVLPT_TIP_LOGITS needs none.  The arguments are checked by the caller (engine.hip).
constexpr int TIP_ROWS = 128;
struct TipPlan {
  int ldn = 0, row_blocks = 0, chunk_rows = 0;
  size_t off_cls = 0, off_at = 0, off_rt = 0, off_z = 0, off_lossp = 0, off_corrp = 0, off_clip = 0, off_cache = 0, ws_bytes = 0;
};
TipPlan tip_plan(int N, int NK, int C, int D, int nb, int na, int mode);
hipError_t launch_tip_logits(const float* F, const float* K, const int32_t* key_ptr, const float* W, float s, float alpha, float beta,
                             int N, int NK, int C, int D, float* logits, hipStream_t st);
hipError_t launch_tip_train_fwd(const float* F, const int32_t* y, const float* K, const int32_t* key_ptr, const float* W, float s,
                                float alpha, float beta, int N, int NK, int C, int D, float* loss, int32_t* correct, float* logits,
                                void* ws, const TipPlan& p, hipStream_t st);
hipError_t launch_tip_train_bwd(const float* F, float alpha, float beta, int N, int NK, int C, int D, float* dK, void* ws,
                                const TipPlan& p, hipStream_t st);
hipError_t launch_tip_search(const float* F, const int32_t* y, const float* K, const int32_t* key_ptr, const float* W, float s,
                             const float* betas, const float* alphas, int N, int NK, int C, int D, int nb, int na, int32_t* counts,
                             void* ws, const TipPlan& p, hipStream_t st);

// ---------------------------------------------------------------- evaluation counts (evaluate.hip; semantics in include/mvlpt_hip.h)
// The arguments are checked by the caller (engine.hip); row indices, task ids, ranges and labels that lie outside their extents are
// clamped or skipped by the kernels, never dereferenced.
struct EvalCountArgs {
  const float* logits; long long ld; int B, C;     // B: rows of logits / labels / task; C: columns
  const long long* label_i; const float* label_f; long long label_ld;    // exactly one of the two label forms
  const int* rows; int n;                          // rows counted: the list (NULL: 0 .. n-1, n == B)
  const int *task, *lo, *hi; int T;                // optional task ranges
  const uint8_t* col_mask;                         // optional: the columns every arg-max runs over
  uint8_t* col_seen;                               // optional: set to 1 for every column with a non-zero target in a counted row
  int64_t *n_true, *n_pred, *n_hit, *n_pred_r, *n_hit_r, *cmat;
};
hipError_t launch_eval_count(const EvalCountArgs& a, hipStream_t s);
// Geometry of one rank call for n selected rows: P = n padded to a power of two; columns of at most MVLPT_EVAL_SORT_TILE items stay in
// LDS (no scratch), longer ones get P items of scratch per workgroup.  ws_bytes never decreases with n at a given (C, cus).
struct EvalRankPlan { int P = 0, grid = 0; bool resident = true; size_t ws_bytes = 0; };
EvalRankPlan eval_rank_plan(int n, int C, int cus);
hipError_t launch_eval_rank_columns(const float* scores, long long ld, int N, int C, const long long* label, const float* target,
                                    long long target_ld, const int* rows, int n, const double* thresholds, long long* n_pos,
                                    long long* n_neg, long long* twice_u, double* interp, int* flags, void* ws, const EvalRankPlan& p,
                                    hipStream_t s);

}  // namespace mvlpt
