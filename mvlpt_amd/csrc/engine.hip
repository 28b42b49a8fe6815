// Host side of libmvlpt_hip.so: the handle (packed frozen CLIP weights, workspaces, saved activations), the
// layer-by-layer orchestration of the hand-written kernels, and the C ABI declared in include/mvlpt_hip.h.
//
// Data layout in HBM (per tower; N sequences of L tokens, width d, token = n*L + i, batch-major):
//   residual stream x      fp32  [N*L, d]      one buffer per LayerNorm input when activations are saved
//                                              (2*layers+1 buffers), a single in-place buffer otherwise
//   h16 (LN output)        16bit [N*L, d]      reused
//   qkv16                  16bit [N*L, 3d]     per layer when saved (attention backward needs Q,K,V)
//   attn16 (attention out) 16bit [N*L, d]      per layer when saved (delta = rowsum(dO*O))
//   lse                    fp32  [N*H*L]       per layer when saved
//   u16 (pre-GELU)         16bit [N*L, 4d]     per layer when saved;  a16 (GELU out) reused
//   backward: dx32 fp32 [N*L,d] (in place through the layers), dx16, dh16, dO16 [N*L,d], du16 [N*L,4d],
//             dqkv16 [N*L,3d], delta [N*H*L]
// Frozen weights: W16 [out,in] (forward Bt operand) and W16^T [in,out] (dX Bt operand), fp32 biases/LN params.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <algorithm>
#include <array>
#include <map>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mvlpt_hip.h"
#include "kernels.h"
#include "jpeg_core.h"

using namespace mvlpt;

// ------------------------------------------------------------------------------------------------ CU-partitioned streams
// A stream made by mvlpt_stream_create_cus only ever gets the compute units of its mask; everything that sizes a grid by
// "resident workgroups" (persistent GEMM, grid-stride LayerNorm) asks stream_cus() instead of the device.  A handful of
// streams per process: a linear scan under a mutex costs nothing next to a launch.  mvlpt_stream_set_cu_cap lowers the figure for ANY
// stream without a mask: the launches then simply use fewer workgroups and leave the other compute units to other streams.

namespace {
struct StreamPart { hipStream_t s; int cus; };
std::mutex g_part_mu;
std::vector<StreamPart> g_parts;
// mvlpt_stream_set_cu_cap: a grid cap on any stream (a multiple of 8; no entry: no cap).  Host state read at enqueue time.
std::vector<StreamPart> g_caps;
int device_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  }
  return cus;
}
}  // namespace
namespace mvlpt {
static int stream_cus_impl(hipStream_t s, bool capped) {
  int cus = 0, cap = 0;
  if (s) {
    std::lock_guard<std::mutex> lk(g_part_mu);
    for (const StreamPart& p : g_parts) if (p.s == s) { cus = p.cus; break; }
    if (capped) for (const StreamPart& p : g_caps) if (p.s == s) { cap = p.cus; break; }
  }
  if (!cus) cus = device_cus();
  return cap > 0 && cap < cus ? cap : cus;
}
int stream_cus(hipStream_t s) { return stream_cus_impl(s, true); }
int stream_cus_nocap(hipStream_t s) { return stream_cus_impl(s, false); }
}  // namespace mvlpt

namespace {

// ------------------------------------------------------------------------------------------------ small utils
// Grow-only workspace.  Growth (a larger batch / class count than anything seen so far) must not stall the streams: work
// that was enqueued on ANY stream may still be using the old block, so it is neither synchronised on nor freed here — it
// is retired and released with the handle (1.5x geometric growth bounds the retired total by 2x the final size; the
// 288 GB of HBM are not the constraint, a device-wide sync in the middle of a step would be).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  std::vector<void*> retired;
  ~DevBuf() {
    if (p) (void)hipFree(p);
    for (void* q : retired) (void)hipFree(q);
  }
  // release the retired blocks; the caller guarantees that nothing enqueued before still uses them (mvlpt_trim)
  size_t trim() {
    size_t n = retired.size();
    for (void* q : retired) (void)hipFree(q);
    retired.clear();
    return n;
  }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    size_t got = std::max(bytes, cap + cap / 2);
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, got);
    if (e != hipSuccess && got > bytes) { got = bytes; e = hipMalloc(&q, got); }      // the slack did not fit: exact size
    if (e != hipSuccess) return e;
    if (p) retired.push_back(p);
    p = q; cap = got;
    return hipSuccess;
  }
};
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
// base == null: a counting pass.  `off` advances as in a carve and every take returns null (carve_ws below).
struct Bump {
  char* base = nullptr; size_t off = 0, cap = 0;
  template <typename T> T* take(size_t count) {
    T* r = base ? (T*)(base + off) : nullptr; off += align256(count * sizeof(T)); return r;
  }
  void* take_bytes(size_t bytes) { return take<char>(bytes); }
};

// Packed frozen weight of one nn.Linear: rows of [W16 (K x 16 bit) | W8 (K bytes, e4m3(W * 2^e8))] with a pitch of 3K/2
// elements, in both orientations (GemmArgs::a_split == 2 reads the fp8 plane, every other GEMM only the 16-bit one).
struct WRef { const void* p; int ld; int e8; };
struct Linear {
  void* w = nullptr; void* wt = nullptr; float* b = nullptr; int out = 0, in = 0;
  int ldw = 0, ldwt = 0, e8 = 0;
  float *fold_s = nullptr, *fold_b = nullptr;   // LayerNorm folding: W gamma and b + W beta of the LayerNorm in front (qkv: ln_1, fc: ln_2)
  // packed residual stream (fp16 image tower without a gradient): round16(W * gamma) [out, in] and its row sums
  void* wg = nullptr; float* fold_sg = nullptr;
  WRef fw() const { return WRef{w, ldw, e8}; }      // forward Bt operand  [out, in]
  WRef fwg() const { return WRef{wg, in, 0}; }
  WRef bw() const { return WRef{wt, ldwt, e8}; }    // dX Bt operand       [in, out]
};
struct LNp { float* g = nullptr; float* b = nullptr; };
struct Block { LNp ln1, ln2; Linear qkv, o, fc, pr; };
struct TowerW { int width = 0, layers = 0, heads = 0; std::vector<Block> blocks; };

// Frozen ModifiedResNet (mvlpt_create_resnet): packed fp16 conv weights [Cout, Kp] (conv.hip) and BatchNorm as the four tensors the
// state dict holds plus the fp32 scale / shift the conv epilogue applies (built once behind a load, prepare_resnet)
struct BNp { float *g = nullptr, *b = nullptr, *m = nullptr, *v = nullptr, *scale = nullptr, *shift = nullptr; };
struct ConvW { void* w = nullptr; int cin = 0, cin_pad = 0, cout = 0, k = 0; BNp bn; };
struct RNBlock { ConvW c1, c2, c3, ds; bool has_ds = false; int stride = 1; };
struct ResNetW {
  bool on = false, ready = false;
  MvlptResNetArch a{};
  ConvW stem[3];
  std::vector<RNBlock> stage[4];
  // AttentionPool2d: positional embedding [T, E] fp32; dense fp16 weights q [E, E], k|v [2E, E], c [out, E] and their fp32 biases
  float* pos = nullptr; void *qw = nullptr, *kvw = nullptr, *cw = nullptr; float *qb = nullptr, *kvb = nullptr, *cb = nullptr;
  bool have[8] = {false, false, false, false, false, false, false, false};      // q, k, v, c weights; q, k, v, c biases
};

struct TowerState {
  bool causal = false;
  bool keep = false;                     // the pass now running writes what a backward reads (lse, u, the skip copies); set by whoever runs the pass
  bool exact = false;                    // split-precision operands + pair-product attention (see DESIGN.md "Precision modes")
  int wide_pitch = 0;                    // split towers: row pitch of a16 / du16 (0: dense)
  int xs = 0;                            // GEMM A operands: 0 single 16-bit, 1 16-bit pair, 2 mixed pair (hi + e5m2 residual byte)
  int N = 0, L = 0, d = 0, H = 0, layers = 0;
  // Gradient length (mvlpt_set_text_grad_len): the leading positions of every sequence a backward processes.  Every gradient buffer
  // (dx32 .. delta) is compact [N, Lg, .]; the saved forward tensors keep the pitch L and are read through the row map
  // saved_rows().  Lg == L: every position (the image tower, and the text tower's default).
  int Lg = 0;
  RowMap saved_rows() const { return Lg != L ? RowMap{Lg, L} : RowMap(); }      // compact gradient row -> row of a saved tensor
  // Shared prefix of a text tower (mvlpt_set_text_shared_prefix; 0: none).  P > 0: the first P positions are the same rows in every
  // class sequence and are evaluated once.  The tower then runs over N = C + 1 "slots" of L rows: slot 0 holds the prefix in its first
  // P rows, slot c + 1 positions P .. of class c, so L and Lg above are the sequence and gradient lengths MINUS P and every row-wise
  // kernel and row map works on the slots unchanged.  Only the attention core (AttnArgs::prefix), the prompt tables (glue.hip) and
  // the last block's compact rows (C of them) know.  kv_part: the attention backward's fp32 dK / dV partials of the prefix keys
  // [N, P, 2d]; part_mul = 2^-s: what they are scaled by when they enter slot 0 (the sum over many classes must stay inside the
  // 16-bit hi plane), undone by the context gather.
  int P = 0; float* kv_part = nullptr; float part_mul = 1.f;
  int seqs() const { return P > 0 ? N - 1 : N; }      // sequences that end in a compact row
  int hw = 64;                           // head width d / H: 64, or a wide-headed image tower's 80 / 96 / 112 / 128 (attention_wide.hip)
  std::vector<float*> x;                 // 2*layers+1 entries (all equal when !saved)
  std::vector<void*> qkv, attn, u;       // per layer (all equal when !saved)
  std::vector<float*> lse;
  void *h16 = nullptr, *a16 = nullptr;
  float* act32 = nullptr;                // exact GELU only: fp32 [T, 4d] between an MLP GEMM and the stand-alone activation pass
  float* dx32 = nullptr; void *dx16 = nullptr, *du16 = nullptr, *dO16 = nullptr, *dqkv16 = nullptr; float* dh32 = nullptr;
  float* delta = nullptr; float* scale_dev = nullptr;
  std::vector<char> skip;                // layer skipped (reference deep-prompt quirk, Appendix A.3)
  // LayerNorm folding (kernels.h): per-row, per-N-tile {sum, sum of squares} of the residual stream in front of ln_1 / ln_2,
  // written by the FC2 / out-projection epilogues; h16 then holds round16(x * gamma) instead of LN(x)
  bool fold = false;
  float* part[2] = {nullptr, nullptr};   // [T][FOLD_NTP][2]
  int nt[2] = {0, 0}, ntp[2] = {0, 0};   // slots in use / slots per row, as the last producer wrote them
  // Activation checkpointing (text tower, mvlpt_set_text_act_ckpt): the plan this forward ran under, seg[i] = first layer of segment
  // i, seg[k] = layers.  Segments 0 .. k-2 kept only their input; the per-layer tensors above are then slots shared by the segments
  // (indexed by the layer's position in its segment) and a backward recomputes each segment into them.  k = 1: nothing shared.
  std::vector<int> seg;
};
constexpr int FOLD_NTP = 8;              // slots per row the buffers are sized for (gemm.hip: FOLD_MAX_NTP)

// The R rows of a tower's last block whose output is read (image: the CLS row of every image; text: the EOT row of every sequence),
// gathered into compact [R, ·] buffers: out-projection, ln_2, the MLP and the closing LayerNorm run on these rows only
// (last_block_fwd / last_block_bwd).  The 16-bit buffers hold hi|lo pairs in a split tower.
struct Compact {
  float *x32 = nullptr, *xm32 = nullptr, *xo32 = nullptr;      // block input, ln_2 input, closing LayerNorm input
  float *out32 = nullptr, *dout32 = nullptr;                   // closing LayerNorm output (the projection's input) and its gradient
  void *a16 = nullptr, *h16 = nullptr, *g16 = nullptr, *u16 = nullptr;      // attention output, ln_2 output, GELU output, pre-GELU
  float *dx32 = nullptr, *dh32 = nullptr; void *dx16 = nullptr, *dO16 = nullptr, *du16 = nullptr;
  float* act32 = nullptr;                // exact GELU only: fp32 [R, 4d] (TowerState::act32 on the compact rows)
};

enum ProfClass { PC_GEMM = 0, PC_ATTN_FWD, PC_ATTN_BWD, PC_LN_FWD, PC_LN_BWD, PC_GLUE, PC_HEAD, PC_ATTN_FWD_IMG, PC_COUNT };
static const char* kProfNames[PC_COUNT] = {"gemm_bt", "attention_fwd", "attention_bwd", "layernorm_fwd", "layernorm_bwd",
                                           "glue", "head_logits_ce", "attention_fwd_image"};
struct ProfRec { int cls; hipEvent_t a, b; double flops, bytes, flops_exec; int M = 0, N = 0, K = 0, epi = -1, split = 0, fold = 0; };

// How the sequences of a text forward are put together: prompts of C classes, prompts of per-group class ranges (CoCoOp is every range
// full; both mvlpt_text_fwd), token ids (mvlpt_text_encode_tokens)
enum class TextKind { Plain, Ranged, Ids };
// The entry that ran the last head forward
enum class HeadKind { Plain, Ranged };

// ---- What the engine remembers of a forward: one record per job (image tower, text tower, head), one phase per record.
// A forward OPENS its record (a fresh one, Phase::None) where it first touches the job's workspace and raises the phase in its last
// statement, so a forward that fails anywhere in between leaves "nothing usable" without a line of its own.  A refusal in front of
// the opening leaves the earlier record as it was.  Readers decide by the phase alone.
//   None      nothing usable (never run, a forward failed or was abandoned)
//   Pending   image only: between mvlpt_image_fwd_begin and mvlpt_image_fwd_resume
//   Done      the forward finished, nothing was saved
//   Saved     saved, no backward yet (the head: every forward; its backward may run any number of times)
//   BwdDone   saved and a backward has run; another one is legal (nothing was checkpointed), and so is mvlpt_set_activation
//   Consumed  text only: a backward under activation checkpointing has overwritten the saved slots
//   entry                          record   from               to
//   image_fwd_begin                image    any but Pending    Pending            (None on failure)
//   image_fwd_resume               image    Pending            Done / Saved       (None on failure)
//   image_fwd_abandon              image    Pending            None
//   image_fwd (ResNet)             image    any                Done               (None on failure)
//   image_bwd                      image    Saved / BwdDone    BwdDone
//   text_fwd / encode_tokens       text     any                Done / Saved       (None on failure)
//   text_bwd                       text     Saved / BwdDone    BwdDone, or Consumed once a checkpointed backward touches the slots
//   logits_fwd / logits_ranged_fwd head     any                Saved              (None on failure)
//   logits_bwd / logits_ranged_bwd head     Saved              Saved              (the forward of its own kind only)
enum class Phase { None, Pending, Done, Saved, BwdDone, Consumed };
static bool bwd_ready(Phase p) { return p == Phase::Saved || p == Phase::BwdDone; }

struct ImageRun {
  Phase phase = Phase::None;
  TowerState st; Compact c;              // carved from vis_ws; c: the CLS-only last block (compact [B,·] rows)
  int B = 0, n_vpt = 0, n_deep = 0;
  bool last_compact = false;             // the last block ran on the compact rows (false: skipped by the deep-prompt quirk)
  bool packed = false, ln1_ready = false, save = false; int next = 0;      // what crosses the begin / resume cut
  // Caller-owned.  mask: the dropout masks this forward took over from mvlpt_set_vpt_dropout (null: none), alive until the last
  // mvlpt_image_bwd of this forward is enqueued.  vpt_deep: alive from mvlpt_image_fwd_begin until mvlpt_image_fwd_resume is enqueued.
  const float *mask = nullptr, *vpt_deep = nullptr;
};
struct TextRun {
  Phase phase = Phase::None;
  TowerState st; Compact c;              // carved from txt_ws; c: the EOT-only last block (compact [C,·] rows)
  TextKind kind = TextKind::Plain;
  int C = 0, L = 0, n_ctx = 0, per_class = 0, n_deep = 0;
  int groups = 0;                        // TextKind::Ranged: the groups, C = sum of the range widths
  // device tables in txt_ws.  range: [lo (groups) | start (groups + 1) | ...] (build_range_table), ids: mvlpt_text_encode_tokens
  int32_t *eot_rows = nullptr, *ctx_pos = nullptr, *range = nullptr, *ids = nullptr;
  // Caller-owned: ctx_deep [n_deep, n_ctx, dt] (MvlptTextJob), read again by the recomputation of a checkpointed backward:
  // alive until the last mvlpt_text_bwd of this forward is enqueued
  const float* ctx_deep = nullptr;
};
struct HeadRun {
  Phase phase = Phase::None;
  HeadKind kind = HeadKind::Plain;       // a backward runs only after the forward of its own name
  int B = 0, C = 0, S = 0; float scale = 0.f;      // HeadKind::Ranged: B = G groups over C classes, S text rows
  float *imn = nullptr, *txn = nullptr, *inorm = nullptr, *tnorm = nullptr;      // carved from head_ws, like the ranged head's tables
  const int32_t *rlo = nullptr, *rstart = nullptr, *rgrp = nullptr;
  // Caller-owned: the class window of mvlpt_logits_fwd (null: none), alive until the last mvlpt_logits_bwd of this forward is enqueued
  const int32_t *lo = nullptr, *hi = nullptr;
};

struct Engine {
  MvlptArch arch{};
  int dt = DT_F16;
  int prec_mode = MVLPT_PREC_SPLIT_GRAD;
  int fold_mode = 2;    // LayerNorm folding: 0 off, 1 image tower, 2 both towers (MVLPT_LN_FOLD, mvlpt_set_ln_fold)
  int act = ACT_QUICKGELU;    // the MLP activation of both towers (mvlpt_set_activation; DESIGN.md "Exact GELU")
  int text_act_ckpt = 1;      // segments of the text tower's activation checkpointing (mvlpt_set_text_act_ckpt; 1: everything is saved)
  // mvlpt_set_text_grad_len: gradient length of the next saving text forwards (0: every position) and the caller's largest EOT position
  int text_grad_len = 0, text_max_eot = 0;
  int text_shared_prefix = 0;      // mvlpt_set_text_shared_prefix: leading positions every class shares (0: off); the next text forward consumes it
  int fold_min_rows = 1024;   // towers with fewer token rows keep the stand-alone LayerNorm (a handful of tiles: nothing to win)
  bool fold_ready = false;
  // packed residual stream: the fp16 image tower without prompts and without a backward carries x as hi (fp16, at the
  // same time the A operand behind every LayerNorm) + one byte instead of fp32 + a 16-bit copy.  MVLPT_RESID_PACKED / mvlpt_set_resid_packed
  int resid_packed = 1;      // MVLPT_RESID_PACKED=0: fp32 stream
  // mvlpt_set_vpt_dropout: [layers, B, n_vpt, d] masks of the visual prompt rows for the NEXT image_fwd (one-shot: the forward
  // validates the geometry, takes the setting over as ImageRun::mask — what ITS backward uses — and clears it, so a stale pointer
  // never reaches another forward or another user of the engine)
  struct VptMask { const float* p = nullptr; int layers = 0, B = 0, n = 0; } vpt_mask;
  bool lo8 = true;      // split towers of MVLPT_PREC_SPLIT_GRAD use the mixed pair (hi + e5m2 residual byte; MVLPT_SPLIT_LO8=0: 16-bit pairs)
  std::string err;
  TowerW vis, txt;
  ResNetW rn;           // rn.on: the image tower is a ModifiedResNet (vis stays empty)
  // vision extras
  void* conv_w = nullptr; int Kp = 0; float* cls_emb = nullptr; float* vpos = nullptr; LNp ln_pre, ln_post;
  float *vproj = nullptr, *vproj_t = nullptr;  // [dv,e] and [e,dv] fp32 (the projections next to the logits stay fp32)
  // text extras
  float* tpos = nullptr; LNp ln_final; float *tproj = nullptr, *tproj_t = nullptr;
  // token embedding [vocab, text_width] fp32: kept only when the caller loads it (mvlpt_text_encode_tokens reads it)
  float* tok_emb = nullptr; int vocab = 0;
  std::vector<void*> owned;               // every weight allocation (freed in destroy)
  DevBuf vis_ws, txt_ws, head_ws, ce_ws, tmp, pp_ws, near_ws, jpeg_ws;
  std::vector<uint8_t> jpeg_meta_host;    // mvlpt_jpeg_decode: descriptors, table sets and segment table (source of the asynchronous upload)
  std::vector<int32_t> jpeg_status_host;  // ... and the initial status words
  ImageRun vrun; TextRun trun; HeadRun hrun;      // the last forward of each job (see Phase)
  std::vector<int32_t> t_range_host, h_range_host;   // host images of the range tables (source of the asynchronous upload)
  std::vector<int32_t> t_ids_host;   // mvlpt_text_encode_tokens: [ids (S * L, trimmed rows) | eot rows (S)], checked on the host
  // profiling
  // mvlpt_debug_checksums: one 64-bit fingerprint per intermediate of the image tower (debug; off by default)
  unsigned long long* dbg_ck = nullptr; int dbg_ck_n = 0; bool dbg_ck_on = false;
  bool prof_on = false, prof_all = false; std::vector<ProfRec> prof; std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
};

thread_local std::string g_create_err;

int fail(Engine* E, int code, const std::string& msg) { if (E) E->err = msg; else g_create_err = msg; return code; }
int hipfail(Engine* E, hipError_t e, const char* what) {
  return fail(E, MVLPT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(E, call) do { hipError_t _e = (call); if (_e != hipSuccess) return hipfail((E), _e, #call); } while (0)

// A workspace is sized by the function that carves it.  `layout` does the takes and stores the pointers; it runs once on a counting
// Bump (the pointers it stores are null then), `ws` reserves that count plus `slack`, and it runs again on the real block.
constexpr size_t kCarveSlack = 4096;
template <typename F> size_t carve_count(F&& layout) { Bump bp; layout(bp); return bp.off; }
template <typename F> int carve_ws(Engine* E, DevBuf& ws, const char* who, size_t slack, F&& layout) {
  HIPCHK(E, ws.reserve(carve_count(layout) + slack));
  Bump bp; bp.base = (char*)ws.p; bp.cap = ws.cap;
  layout(bp);
  if (bp.off > bp.cap) return fail(E, MVLPT_ERR_STATE, std::string(who) + ": the workspace carve exceeds its reservation");
  return 0;
}

// Two events of the profiling pool, which grows by 512 up to 65 536 events; false: none left (the launch then goes unrecorded)
bool take_events(Engine* E, hipEvent_t* a, hipEvent_t* b) {
  if (E->ev_used + 2 > E->ev_pool.size() && E->ev_pool.size() < 65536)
    for (int i = 0; i < 512; ++i) { hipEvent_t ev; if (hipEventCreate(&ev) != hipSuccess) break; E->ev_pool.push_back(ev); }
  if (E->ev_used + 2 > E->ev_pool.size()) return false;
  *a = E->ev_pool[E->ev_used++]; *b = E->ev_pool[E->ev_used++];
  return true;
}

struct ProfScope {
  Engine* E; hipStream_t s; bool on = false; hipEvent_t b{};
  ProfScope(Engine* E_, hipStream_t s_, int cls, double flops, double bytes) : E(E_), s(s_) {
    if (!E || !E->prof_on || !E->prof_all) return;   // marker events cost ~1.5 us each: only in the full-breakdown mode
    hipEvent_t a{};
    if (!take_events(E, &a, &b)) return;
    (void)hipEventRecord(a, s);
    E->prof.push_back(ProfRec{cls, a, b, flops, bytes, flops});
    on = true;
  }
  ~ProfScope() { if (on) (void)hipEventRecord(b, s); }
};

constexpr int DBG_CK_MAX = 256;
static void dbg_ck(Engine* E, const void* p, size_t bytes, hipStream_t s) {
  if (!E->dbg_ck_on || !E->dbg_ck || E->dbg_ck_n >= DBG_CK_MAX) return;
  (void)launch_checksum(p, bytes, E->dbg_ck + E->dbg_ck_n++, s);
}

// the single-operand attention forward (the headline's image tower), timed like the GEMMs by its own dispatch timestamps whenever
// profiling is on (class "attention_fwd_image": bench.py's roofline.image_attention_fwd)
static hipError_t attn_fwd_timed(Engine* E, const AttnArgs& a, double flops, double bytes, hipStream_t s) {
  hipEvent_t ea = nullptr, eb = nullptr;
  if (E && E->prof_on && !E->prof_all && take_events(E, &ea, &eb))
    E->prof.push_back(ProfRec{PC_ATTN_FWD_IMG, ea, eb, flops, bytes, flops});
  return launch_attn_fwd(E->dt, a, s, ea, eb);
}

// ------------------------------------------------------------------------------------------------ kernel wrappers
// What a launch's arguments are is decided in kernels.h: the call sites below fill the launcher's struct by field name, and the wrappers
// add only what the engine knows, the compute dtype, the packed weight (WRef -> Bt / ldb / w8_exp), the mixed-pair output rule and
// the profile record.  gemm_args / ln_args / ln_bwd_args: the fields every such launch has.
GemmArgs gemm_args(const void* A, int M, int N, int K, void* out) {
  GemmArgs g;
  g.A = A; g.M = M; g.N = N; g.K = K; g.out = out;
  return g;
}
hipError_t gemm(Engine* E, int epi, GemmArgs g, WRef Bt, hipStream_t s, int dtype = -1) {
  g.Bt = Bt.p; g.ldb = Bt.ld; g.w8_exp = Bt.e8;
  g.out_lo8 = (g.a_split == 2 && (epi == EPI_GELU_SPLIT || epi == EPI_GELUBWD_SPLIT)) ? 1 : 0;
  const int dt = dtype >= 0 ? dtype : E->dt;
  const int M = g.M, N = g.N, K = g.K, a_split = g.a_split;
  const double ob = (epi == EPI_RESIDP_LN) ? 6.0 : (epi == EPI_RESID32) ? 8.0 : (epi == EPI_RESID32_LN) ? 8.0 + 2.0 * (a_split ? 1.5 : 1.0) : ((epi == EPI_STORE32 || epi == EPI_STORE_SPLIT) ? 4.0 : ((epi == EPI_GELUBWD || epi == EPI_GELU_SPLIT) ? 4.0 :
                    (epi == EPI_GELUBWD_SPLIT ? 6.0 : 2.0)));
  // the dominant kernel is timed by its own dispatch (start/stop timestamps of the AQL packet): no marker packets
  hipEvent_t ea = nullptr, eb = nullptr;
  if (E && E->prof_on && take_events(E, &ea, &eb)) {
    // flops = ALGORITHMIC (what the reference's fp32 GEMM does: 2MNK); the split-precision modes execute twice that
    // (16-bit pair) or 1.5x in 16-bit-MFMA time (mixed pair: the residual term runs on the fp8 MFMA at twice the rate)
    const double xa = a_split == 2 ? 1.5 : (a_split ? 2.0 : 1.0);
    E->prof.push_back(ProfRec{PC_GEMM, ea, eb, 2.0 * M * N * K,
                              2.0 * ((double)M * K * xa + (double)N * K * (a_split == 2 ? 1.5 : 1.0)) + ob * M * N + (g.out2 ? 2.0 * M * N : 0),
                              2.0 * M * N * K * xa, M, N, K, epi, a_split, g.fold_part ? 1 : 0});
  }
  return launch_gemm(dt, epi, g, s, ea, eb);
}
// (every row of x in order: row_idx null, row_mul 1)
LnFwdArgs ln_args(const float* x, const LNp& p, void* y, int rows, int d) {
  LnFwdArgs a;
  a.x = x; a.gamma = p.g; a.beta = p.b; a.y = y; a.rows = rows; a.d = d;
  return a;
}
hipError_t ln_fwd(Engine* E, int out_dt, const LnFwdArgs& a, hipStream_t s) {
  ProfScope ps(E, s, PC_LN_FWD, 8.0 * a.rows * a.d, (double)a.rows * a.d * (4.0 + (out_dt == DT_F32 ? 4.0 : 2.0)));
  return launch_ln_fwd(out_dt, a, s);
}
// (dy fp32: the dX GEMMs that feed a LayerNorm backward store fp32)
LnBwdArgs ln_bwd_args(const float* dy, const float* x, const LNp& p, float* out32, int rows, int d) {
  LnBwdArgs a;
  a.dy = dy; a.dy_dtype = DT_F32; a.x = x; a.gamma = p.g; a.out32 = out32; a.rows = rows; a.d = d;
  return a;
}
hipError_t ln_bwd(Engine* E, const LnBwdArgs& a, hipStream_t s) {
  ProfScope ps(E, s, PC_LN_BWD, 14.0 * a.rows * a.d,
               (double)a.rows * a.d * ((a.dy_dtype == DT_F32 ? 4.0 : 2.0) + 4.0 + (a.resid ? 4.0 : 0.0) + 4.0 + (a.out16 ? 2.0 : 0.0)));
  return launch_ln_bwd(E->dt, a, s);
}

// ------------------------------------------------------------------------------------------------ tower workspace
// The segments of torch.utils.checkpoint.checkpoint_sequential(blocks, segments, x), as the reference cuts its text tower
// (trainers/mvlpt.py:119-121): k = min(max(segments, 1), layers) segments, the first k - 1 of layers / k blocks each (checkpointed),
// the last one takes the rest (saved).  Returns the first layer of every segment and, behind them, `layers`.
std::vector<int> ckpt_plan(int layers, int segments) {
  const int k = std::min(std::max(segments, 1), std::max(layers, 1)), size = layers / k;
  std::vector<int> seg((size_t)k + 1);
  for (int i = 0; i < k; ++i) seg[i] = i * size;
  seg[k] = layers;
  return seg;
}
// row pitch (16-bit elements) of the pair tensors between the two MLP GEMMs ([T, 2 * 4d]: a16, du16; GemmArgs::lda / ldo): rows
// whose dense pitch is a multiple of 4 KiB get 128 bytes more (every CLIP width: 16 d bytes)
int wide_pitch(int cols) {
  return (4 * cols) % 4096 == 0 ? 2 * cols + 64 : 0;
}
// The tower's buffers; on a counting Bump (carve_ws) the tower's size.
// `exact` (split-precision mode): every 16-bit operand buffer holds a hi|lo pair (twice the columns) and QKV / dO are fp32
// segments > 1 (a saving text tower under activation checkpointing): the per-layer tensors shrink to the m slots of the largest
// segment (the last one), the k segment inputs stay (x[0] and k - 1 boundary buffers)
// gelu (Engine::act == ACT_GELU): one more fp32 [T, 4d] buffer, the scratch of the stand-alone activation pass
// Lg (TowerState::Lg; 0: L): the gradient buffers hold N * Lg rows
struct TowerShape {
  int N = 0, L = 0;
  bool save = false, causal = false, exact = false;
  int xs = 0;            // the pair format of an `exact` tower (split_kind)
  bool gelu = false;
  int segments = 1, Lg = 0, P = 0;
};
void carve_tower(Bump& bp, const TowerW& W, TowerState& st, const TowerShape& t) {
  const int N = t.N, L = t.L, Lg = t.Lg, P = t.P, xs = t.xs, segments = t.segments;
  const bool save = t.save, causal = t.causal, exact = t.exact, gelu = t.gelu;
  const size_t T = (size_t)N * L, d = W.width, H = W.heads, X = exact ? 2 : 1; const int nl = W.layers;
  st = TowerState();
  st.P = P;      // (N, L, Lg are the slot figures then: TowerState::P)
  st.N = N; st.L = L; st.Lg = Lg > 0 ? Lg : L; st.d = (int)d; st.H = (int)H; st.hw = (int)(d / H); st.layers = nl; st.causal = causal; st.exact = exact;
  st.xs = exact ? xs : 0;
  st.seg = ckpt_plan(nl, save ? segments : 1);
  const int k = (int)st.seg.size() - 1;
  st.x.resize(2 * nl + 1); st.qkv.resize(nl); st.attn.resize(nl); st.u.resize(nl); st.lse.resize(nl); st.skip.assign(nl, 0);
  float* x0 = bp.take<float>(T * d);
  if (k > 1) {
    // layer l at position j of its segment: its input is the segment's input (x0, or the boundary buffer the block in front of
    // it wrote) at j = 0 and slot j otherwise; x[2 l + 1] and the 16-bit tensors are slot j.  The largest segment is the last one.
    const int m = st.seg[k] - st.seg[k - 1];
    std::vector<float*> xin(m), xmid(m); std::vector<void*> qkv(m), attn(m), u(m); std::vector<float*> lse(m);
    for (int j = 0; j < m; ++j) { xin[j] = j ? bp.take<float>(T * d) : nullptr; xmid[j] = bp.take<float>(T * d); }
    st.x[2 * nl] = x0;      // the last block runs on compact rows: nothing is written here
    for (int i = 0; i < k; ++i) {
      float* in = i ? bp.take<float>(T * d) : x0;
      for (int l = st.seg[i]; l < st.seg[i + 1]; ++l) {
        const int j = l - st.seg[i];
        st.x[2 * l] = j ? xin[j] : in; st.x[2 * l + 1] = xmid[j];
      }
    }
    st.h16 = bp.take_bytes(T * d * 2 * X);
    for (int j = 0; j < m; ++j) {
      qkv[j] = bp.take_bytes(T * 3 * d * 2 * X); attn[j] = bp.take_bytes(T * d * 2 * X);
      lse[j] = bp.take<float>((size_t)N * H * L); u[j] = bp.take_bytes(T * 4 * d * 2);
    }
    for (int i = 0; i < k; ++i)
      for (int l = st.seg[i]; l < st.seg[i + 1]; ++l) {
        const int j = l - st.seg[i];
        st.qkv[l] = qkv[j]; st.attn[l] = attn[j]; st.lse[l] = lse[j]; st.u[l] = u[j];
      }
  } else {
    for (int i = 0; i < 2 * nl + 1; ++i) st.x[i] = (save && i > 0) ? bp.take<float>(T * d) : x0;
    st.h16 = bp.take_bytes(T * d * 2 * X);
    for (int l = 0; l < nl; ++l) {
      const bool fresh = save || l == 0;
      st.qkv[l] = fresh ? bp.take_bytes(T * 3 * d * 2 * X) : st.qkv[0];
      st.attn[l] = fresh ? bp.take_bytes(T * d * 2 * X) : st.attn[0];
      st.lse[l] = fresh ? bp.take<float>((size_t)N * H * L) : st.lse[0];
      st.u[l] = fresh ? bp.take_bytes(T * 4 * d * 2) : st.u[0];
    }
  }
  st.a16 = bp.take_bytes(T * (4 * d * 2 * X + 128));
  st.wide_pitch = exact ? wide_pitch(4 * (int)d) : 0;
  st.part[0] = bp.take<float>(T * FOLD_NTP * 2); st.part[1] = bp.take<float>(T * FOLD_NTP * 2);
  if (save) {
    const size_t Tg = (size_t)N * st.Lg;
    st.dx32 = bp.take<float>(Tg * d);
    st.dx16 = bp.take_bytes(Tg * d * 2 * X); st.dh32 = bp.take<float>(Tg * d); st.dO16 = bp.take_bytes(Tg * d * 2 * X);
    st.du16 = bp.take_bytes(Tg * (4 * d * 2 * X + 128)); st.dqkv16 = bp.take_bytes(Tg * 3 * d * 2 * X);
    st.delta = bp.take<float>((size_t)N * H * st.Lg);
    if (P > 0) st.kv_part = bp.take<float>((size_t)N * P * 2 * d);
    st.scale_dev = bp.take<float>(4);   // {scale, 1/scale, amax scratch, pad}
  }
  if (gelu) st.act32 = bp.take<float>(T * 4 * d);
}

// which pair format a split tower uses: the default mode carries the residual as one e5m2 byte (GemmArgs::a_split == 2);
// MVLPT_PREC_SPLIT_ALL (PREC = "fp32": as exact as this engine gets) keeps 16-bit pairs everywhere
int split_kind(const Engine* E) { return (E->prec_mode == MVLPT_PREC_SPLIT_ALL || !E->lo8) ? 1 : 2; }

// Attention core of layer l, all rows or (q_rows > 0) only queries 0..q_rows-1 of every sequence; lse is kept when the pass keeps its
// activations (st.keep).  Split towers (st.xs): qkv pair [T,6d] -> O as a hi|lo pair [T,2d].  Single operands: `timed` (the full-width blocks)
// adds the dispatch-timestamp record of attn_fwd_timed.
int attn_fwd(Engine* E, TowerState& st, int l, int q_rows, bool timed, hipStream_t s) {
  const double T = (double)st.N * st.L, rows = q_rows > 0 ? (double)q_rows : (double)st.L;
  const double fl = 4.0 * rows * st.L * (double)st.hw * st.N * st.H * (st.causal ? 0.5 : 1.0);
  AttnArgs a;
  a.qkv = st.qkv[l]; a.out = st.attn[l]; a.lse = st.keep ? st.lse[l] : nullptr;
  a.N = st.seqs(); a.L = st.L + st.P; a.H = st.H; a.causal = st.causal ? 1 : 0;      // (shared prefix: slots, TowerState::P)
  a.q_rows = q_rows; a.prefix = st.P; a.fmt = st.xs;
  if (st.hw != 64) {      // a wide-headed image tower: frozen, prompt-free, forward-only on single operands (kRefuseWide)
    if (st.xs || st.causal || st.keep) return fail(E, MVLPT_ERR_STATE, "wide-headed attention: single operands, non-causal, nothing saved");
    ProfScope ps(E, s, PC_ATTN_FWD, fl, T * st.d * 2.0 * (q_rows > 0 ? 2.0 : 4.0));
    HIPCHK(E, launch_attn_fwd_wide(E->dt, a, st.hw, s));
    return 0;
  }
  const double by = st.xs ? T * st.d * 16.0 : T * st.d * 2.0 * (q_rows > 0 ? 2.0 : 4.0);
  ProfScope ps(E, s, PC_ATTN_FWD, fl, by);
  HIPCHK(E, timed && !st.xs ? attn_fwd_timed(E, a, fl, by, s) : launch_attn_fwd(E->dt, a, s));
  return 0;
}
// Attention backward of layer l: dO16 -> dqkv16 at full width, or (cls, single operands only) the backward of query 0 of every
// sequence on the compact rows of the last image block
int attn_bwd(Engine* E, TowerState& st, int l, const Compact* cls, hipStream_t s) {
  const double T = (double)st.N * st.L, cz = st.causal ? 0.5 : 1.0;
  if (cls) {
    ProfScope ps(E, s, PC_ATTN_BWD, 10.0 * st.L * 64.0 * st.N * st.H * cz, T * st.d * 2.0 * 5.0);
    HIPCHK(E, launch_attn_bwd_cls(E->dt, st.qkv[l], cls->a16, cls->dO16, st.lse[l], st.dqkv16, st.N, st.L, st.H, s));
    return 0;
  }
  // (the positions that carry a gradient: st.Lg of the st.L saved ones)
  const double fl = 14.0 * st.Lg * st.Lg * 64.0 * st.N * st.H * cz, Tg = (double)st.N * st.Lg;
  AttnBwdArgs a;
  a.qkv = st.qkv[l]; a.out = st.attn[l]; a.dout = st.dO16; a.lse = st.lse[l]; a.delta = st.delta; a.dqkv = st.dqkv16;
  a.N = st.seqs(); a.L = st.Lg + st.P; a.Ls = st.L + st.P; a.H = st.H; a.causal = st.causal ? 1 : 0; a.fmt = st.xs;
  a.prefix = st.P; a.kv_part = st.kv_part; a.part_mul = st.part_mul;      // (shared prefix: one more launch, the reduction of kv_part)
  ProfScope ps(E, s, PC_ATTN_BWD, fl, st.xs ? Tg * st.d * 32.0 : Tg * st.d * 2.0 * 8.0);
  HIPCHK(E, launch_attn_bwd(E->dt, a, s));
  return 0;
}

// ---- LayerNorm folding (kernels.h GemmArgs::ln_* / fold_*): the residual GEMM in front of a LayerNorm writes
// round16(x * gamma) into h16 and per-row partial sums; the GEMM behind it applies mean / rstd in its epilogue.
// which = 0: the LayerNorm is ln_1 (producer: FC2 of the previous block), 1: ln_2 (producer: this block's out-projection).
// fold_producer: `g` (M, N, K set) becomes the producer when its launch can be one, and the tower remembers the slots it fills;
// fold_consumer: `g` reads them, colsum = W gamma of its weight (Linear::fold_s, or fold_sg on the packed stream).
bool fold_producer(Engine* E, TowerState& st, int which, const LNp& ln, hipStream_t s, GemmArgs& g) {
  if (!st.fold) return false;
  GemmArgs q;      // (the shape and the operand format: all the launcher's routing reads)
  q.M = g.M; q.N = g.N; q.K = g.K; q.a_split = st.xs;
  const int bn = gemm_tile_n(E->dt, EPI_RESID32_LN, q, s);      // the launcher's N-tile for this problem on this stream
  if (bn <= 0 || g.N % bn) return false;
  const int nt = g.N / 128, ntp = (nt + 1) & ~1;          // one slot per 128 output columns, whatever the tile geometry
  if (ntp > FOLD_NTP) return false;
  g.ln_gamma = ln.g; g.ln_x16 = st.h16; g.ln_split = st.xs; g.ln_part = st.part[which]; g.ln_ntp = ntp;
  st.nt[which] = nt; st.ntp[which] = ntp;
  return true;
}
void fold_consumer(const TowerState& st, int which, const float* colsum, GemmArgs& g) {
  g.fold_part = st.part[which]; g.fold_colsum = colsum; g.fold_ntp = st.ntp[which]; g.fold_nt = st.nt[which];
}

// ---- The MLP's activation (Engine::act).  QuickGELU lives in the GEMM epilogues (EPI_GELU* / EPI_GELUBWD*).  The exact GELU of a
// checkpoint trained with nn.GELU is a pass of its own (activation.hip): the GEMM stores fp32 into `scratch` (EPI_STORE32: the activation
// sees u = acc + bias unrounded) and the pass writes the A operand of the next GEMM in the tower's format at the pitch g.ldo.
// mlp_up: g.out = act(g.A fc^T + g.bias) in the format g.a_split, u16 (optional) = the saved pre-activation.  g may be the consumer
// side of a folded ln_2 (QuickGELU only)
int mlp_up(Engine* E, GemmArgs g, WRef fc, void* u16, float* scratch, hipStream_t s) {
  if (E->act == ACT_QUICKGELU) {
    g.out2 = u16;
    HIPCHK(E, gemm(E, g.a_split ? EPI_GELU_SPLIT : EPI_GELU, g, fc, s));
    return 0;
  }
  if (g.fold_part || !scratch) return fail(E, MVLPT_ERR_STATE, "exact GELU: the MLP-up GEMM has no folded form and needs its scratch");
  const int M = g.M, N = g.N, xs = g.a_split;
  ActArgs a;
  a.in = scratch; a.out = g.out; a.fmt = xs; a.ldo = g.ldo; a.u16 = u16; a.M = M; a.N = N;
  g.out = scratch; g.ldo = 0;
  HIPCHK(E, gemm(E, EPI_STORE32, g, fc, s));
  ProfScope ps(E, s, PC_GLUE, 10.0 * M * N, (double)M * N * (4.0 + (xs == 1 ? 4.0 : xs ? 3.0 : 2.0) + (u16 ? 2.0 : 0.0)));
  HIPCHK(E, launch_act_fwd(E->dt, E->act, a, s));
  return 0;
}
// mlp_up_bwd: g.out = (g.A prt^T) * act'(g.aux), the gradient at the pre-activation in the format g.a_split; g.aux is the saved u16,
// read through g.aux_rows
int mlp_up_bwd(Engine* E, GemmArgs g, WRef prt, float* scratch, hipStream_t s) {
  if (E->act == ACT_QUICKGELU) {
    HIPCHK(E, gemm(E, g.a_split ? EPI_GELUBWD_SPLIT : EPI_GELUBWD, g, prt, s));
    return 0;
  }
  if (!scratch) return fail(E, MVLPT_ERR_STATE, "exact GELU: the saved state was carved without the activation scratch");
  const int M = g.M, N = g.N, xs = g.a_split;
  ActArgs a;
  a.in = scratch; a.out = g.out; a.fmt = xs; a.ldo = g.ldo; a.u16 = const_cast<void*>(g.aux); a.M = M; a.N = N; a.u_rows = g.aux_rows;
  g.out = scratch; g.ldo = 0; g.aux = nullptr; g.aux_rows = RowMap();
  HIPCHK(E, gemm(E, EPI_STORE32, g, prt, s));
  ProfScope ps(E, s, PC_GLUE, 14.0 * M * N, (double)M * N * (6.0 + (xs == 1 ? 4.0 : xs ? 3.0 : 2.0)));
  HIPCHK(E, launch_act_bwd(E->dt, E->act, a, s));
  return 0;
}

// ResidualAttentionBlock.forward (clip/model.py:185-188) on token buffers.  Split towers (st.xs; towers that carry a gradient, and every
// tower under MVLPT_PREC_SPLIT_ALL): every GEMM A operand is a 16-bit hi|lo pair (~22 bits), the attention core runs in fp32, and the
// pair rows between the two MLP GEMMs have the pitch st.wide_pitch.
// ln1_folded: h16 / part[0] already hold this block's ln_1 input in folded form (written by the previous block's FC2);
// next_ln1: the LayerNorm the block's output goes into next, when that one may be folded; *produced: it was.
int block_fwd(Engine* E, const TowerW& W, TowerState& st, int l, hipStream_t s, bool ln1_folded = false, const LNp* next_ln1 = nullptr,
              bool* produced = nullptr) {
  if (produced) *produced = false;
  const Block& B = W.blocks[l];
  const int T = st.N * st.L, d = st.d, xs = st.xs, wp = st.wide_pitch;
  float* xin = st.x[2 * l]; float* xmid = st.x[2 * l + 1]; float* xout = st.x[2 * l + 2];
  LnFwdArgs ln = ln_args(xin, B.ln1, st.h16, T, d);
  ln.split = xs;
  GemmArgs q = gemm_args(st.h16, T, 3 * d, d, st.qkv[l]);
  q.a_split = xs; q.bias = ln1_folded ? B.qkv.fold_b : B.qkv.b;
  if (ln1_folded) fold_consumer(st, 0, B.qkv.fold_s, q);
  else HIPCHK(E, ln_fwd(E, E->dt, ln, s));
  HIPCHK(E, gemm(E, xs ? EPI_STORE_SPLIT : EPI_STORE16, q, B.qkv.fw(), s));
  if (int rc = attn_fwd(E, st, l, 0, true, s)) return rc;
  GemmArgs o = gemm_args(st.attn[l], T, d, d, xmid);
  o.a_split = xs; o.bias = B.o.b; o.resid = xin;
  // (exact GELU: ln_2 stays a pass of its own: its consumer stores fp32, which has no folded epilogue; ln_1 is folded as ever)
  const bool p2 = E->act == ACT_QUICKGELU && fold_producer(E, st, 1, B.ln2, s, o);
  HIPCHK(E, gemm(E, p2 ? EPI_RESID32_LN : EPI_RESID32, o, B.o.fw(), s));
  GemmArgs fc = gemm_args(st.h16, T, 4 * d, d, st.a16);
  fc.a_split = xs; fc.bias = p2 ? B.fc.fold_b : B.fc.b; fc.ldo = wp;
  ln.x = xmid; ln.gamma = B.ln2.g; ln.beta = B.ln2.b;
  if (p2) fold_consumer(st, 1, B.fc.fold_s, fc);
  else HIPCHK(E, ln_fwd(E, E->dt, ln, s));
  if (int rc = mlp_up(E, fc, B.fc.fw(), st.keep ? st.u[l] : nullptr, st.act32, s)) return rc;
  GemmArgs pr = gemm_args(st.a16, T, d, 4 * d, xout);
  pr.a_split = xs; pr.bias = B.pr.b; pr.resid = xmid; pr.lda = wp;
  const bool p1 = next_ln1 && fold_producer(E, st, 0, *next_ln1, s, pr);
  HIPCHK(E, gemm(E, p1 ? EPI_RESID32_LN : EPI_RESID32, pr, B.pr.fw(), s));
  if (produced) *produced = p1;
  return 0;
}

// block_fwd on the PACKED residual stream (common.h respk_*, kernels.h EPI_RESIDP_LN): fp16 tower, single operands (st.xs == 0), nothing saved,
// both LayerNorms folded.  The stream lives in st.x[0] as hi [T,d] fp16 | lo [T,d] bytes and is updated in place; the hi plane is
// the A operand of the QKV / MLP-up GEMMs, whose weights carry the LayerNorm's gamma (Linear::wg).  part[0] holds the row
// statistics of the stream on entry (the previous block's FC2, or the pack kernel in front of block 0).
int block_fwd_packed(Engine* E, const TowerW& W, TowerState& st, int l, hipStream_t s) {
  const Block& B = W.blocks[l];
  const int T = st.N * st.L, d = st.d;
  if (E->act != ACT_QUICKGELU) return fail(E, MVLPT_ERR_STATE, "packed residual stream: QuickGELU only (the image forward does not take it under the exact GELU)");
  void* hi = st.x[0];
  uint8_t* lo = (uint8_t*)st.x[0] + (size_t)T * d * 2;
  GemmArgs q = gemm_args(hi, T, 3 * d, d, st.qkv[l]);
  q.bias = B.qkv.fold_b;
  fold_consumer(st, 0, B.qkv.fold_sg, q);
  HIPCHK(E, gemm(E, EPI_STORE16, q, B.qkv.fwg(), s));
  dbg_ck(E, st.qkv[l], (size_t)T * 3 * d * 2, s);
  if (int rc = attn_fwd(E, st, l, 0, true, s)) return rc;
  dbg_ck(E, st.attn[l], (size_t)T * d * 2, s);
  GemmArgs o = gemm_args(st.attn[l], T, d, d, hi);
  o.bias = B.o.b; o.rp_hi_in = hi; o.rp_lo_in = lo; o.rp_lo_out = lo;
  if (!fold_producer(E, st, 1, B.ln2, s, o)) return fail(E, MVLPT_ERR_STATE, "packed residual stream: out-projection cannot produce the ln_2 statistics");
  HIPCHK(E, gemm(E, EPI_RESIDP_LN, o, B.o.fw(), s));
  dbg_ck(E, hi, (size_t)T * d * 3, s); dbg_ck(E, o.ln_part, (size_t)T * o.ln_ntp * 8, s);
  GemmArgs fc = gemm_args(hi, T, 4 * d, d, st.a16);
  fc.bias = B.fc.fold_b;
  fold_consumer(st, 1, B.fc.fold_sg, fc);
  HIPCHK(E, gemm(E, EPI_GELU, fc, B.fc.fwg(), s));
  dbg_ck(E, st.a16, (size_t)T * 4 * d * 2, s);
  GemmArgs pr = gemm_args(st.a16, T, d, 4 * d, hi);
  pr.bias = B.pr.b; pr.rp_hi_in = hi; pr.rp_lo_in = lo; pr.rp_lo_out = lo;
  if (!fold_producer(E, st, 0, B.ln1, s, pr)) return fail(E, MVLPT_ERR_STATE, "packed residual stream: MLP down-projection cannot produce the ln_1 statistics");
  HIPCHK(E, gemm(E, EPI_RESIDP_LN, pr, B.pr.fw(), s));
  dbg_ck(E, hi, (size_t)T * d * 3, s); dbg_ck(E, pr.ln_part, (size_t)T * pr.ln_ntp * 8, s);
  return 0;
}

// dX-only backward of one block: dx32/dx16 hold d(block output) on entry and d(block input) on exit
// The gradient buffers hold the T = N * Lg rows that carry a gradient (TowerState::Lg); the saved u and x are read through the row
// map st.saved_rows().
int block_bwd(Engine* E, const TowerW& W, TowerState& st, int l, hipStream_t s) {
  const Block& B = W.blocks[l];
  const int T = st.N * st.Lg, d = st.d, xs = st.xs, wp = st.wide_pitch;
  GemmArgs up = gemm_args(st.dx16, T, 4 * d, d, st.du16);
  up.a_split = xs; up.aux = st.u[l]; up.aux_rows = st.saved_rows(); up.ldo = wp;
  if (int rc = mlp_up_bwd(E, up, B.pr.bw(), st.act32, s)) return rc;
  // the dX GEMMs that feed a LayerNorm backward store fp32 (one 16-bit rounding less per half layer)
  GemmArgs fc = gemm_args(st.du16, T, d, 4 * d, st.dh32);
  fc.a_split = xs; fc.lda = wp;
  HIPCHK(E, gemm(E, EPI_STORE32, fc, B.fc.bw(), s));
  LnBwdArgs ln = ln_bwd_args(st.dh32, st.x[2 * l + 1], B.ln2, st.dx32, T, d);
  ln.resid = st.dx32; ln.out16 = st.dx16; ln.split = xs; ln.x_rows = st.saved_rows();
  HIPCHK(E, ln_bwd(E, ln, s));
  GemmArgs o = gemm_args(st.dx16, T, d, d, st.dO16);
  o.a_split = xs;
  HIPCHK(E, gemm(E, xs ? EPI_STORE_SPLIT : EPI_STORE16, o, B.o.bw(), s));
  if (int rc = attn_bwd(E, st, l, nullptr, s)) return rc;
  GemmArgs q = gemm_args(st.dqkv16, T, d, 3 * d, st.dh32);
  q.a_split = xs;
  HIPCHK(E, gemm(E, EPI_STORE32, q, B.qkv.bw(), s));
  ln.x = st.x[2 * l]; ln.gamma = B.ln1.g;
  HIPCHK(E, ln_bwd(E, ln, s));
  return 0;
}

// ---- The last block of a tower, evaluated on the rows that are read (Compact): ln_1, QKV and the attention still see every token
// (keys / values), then out-proj, ln_2, the MLP and the closing LayerNorm run on the R = st.N compact rows instead of R * L: ~20/24
// of the layer's GEMM FLOPs vanish, in the forward and, when the tower has a backward, in the backward as well.
// u16 is never a pair and still taken at pair width: mvlpt_text_workspace_bytes publishes it at that width (see kTextSlack)
void carve_compact(Bump& bp, Compact& c, size_t R, size_t d, size_t X, bool gelu) {
  c = Compact();
  for (float** p : {&c.out32, &c.dout32, &c.x32, &c.xm32, &c.xo32, &c.dx32, &c.dh32}) *p = bp.take<float>(R * d);
  for (void** p : {&c.a16, &c.h16, &c.dx16, &c.dO16}) *p = bp.take_bytes(R * d * 2 * X);
  c.g16 = bp.take_bytes(R * d * 8 * X); c.u16 = bp.take_bytes(R * d * 8 * X); c.du16 = bp.take_bytes(R * d * 8 * X);
  if (gelu) c.act32 = bp.take<float>(R * 4 * d);
}
// compact row r <-> token row rows[r] or (rows == null) row 0 of sequence r; scatter: compact -> full width
// A gather reads the saved tensors (pitch st.L).  A scatter writes the gradient buffers, which hold st.Lg rows of every sequence while
// `rows` goes on naming saved rows: st.saved_rows()
hipError_t move_rows(const TowerState& st, const void* src, void* dst, const int32_t* rows, int R, size_t row_bytes, int scatter, hipStream_t s) {
  const RowMap far = scatter ? st.saved_rows() : RowMap();
  if (rows) return launch_copy_rows(src, dst, rows, R, (int)row_bytes, scatter, s, far);
  if (far.seq) return hipErrorInvalidValue;
  return launch_copy_rows_strided(src, dst, R, scatter ? row_bytes : st.L * row_bytes, scatter ? st.L * row_bytes : row_bytes, (int)row_bytes, s);
}
// Which rows a tower's last block is evaluated on and what closes it.
// Image: only x[:, 0, :] of the last block is read (trainers/mvlpt.py:88), rows == null, and only the CLS query runs (q_rows = 1).
// Text: only x[c, eot_c] (trainers/mvlpt.py:126-128), rows = eot_rows, every query runs (q_rows = 0).
// ln_close: ln_post / ln_final, into c.out32.
struct LastRows { const int32_t* rows; int q_rows; const LNp& ln_close; };
// packed: the image tower's packed stream.  The image tower (rows == null) also leaves mvlpt_debug_checksums fingerprints.
int last_block_fwd(Engine* E, const TowerW& W, TowerState& st, Compact& c, const LastRows& lr, bool packed, bool ln1_ready, hipStream_t s) {
  const int l = st.layers - 1, T = st.N * st.L, R = st.seqs(), d = st.d;
  const int xs = st.xs;                 // split-precision operands (hi|lo pairs, twice the columns) + pair-product attention
  const size_t X = xs ? 2 : 1;
  const bool ck = !lr.rows;
  const Block& Bk = W.blocks[l];
  float* xin = st.x[2 * l];
  LnFwdArgs ln = ln_args(xin, Bk.ln1, st.h16, T, d);
  ln.split = xs;
  GemmArgs q = gemm_args(packed ? (void*)st.x[0] : st.h16, T, 3 * d, d, st.qkv[l]);
  q.a_split = xs; q.bias = ln1_ready ? Bk.qkv.fold_b : Bk.qkv.b;
  // (packed: A = the stream's hi plane, gamma inside the weight)
  if (ln1_ready) fold_consumer(st, 0, packed ? Bk.qkv.fold_sg : Bk.qkv.fold_s, q);
  else HIPCHK(E, ln_fwd(E, E->dt, ln, s));
  HIPCHK(E, gemm(E, xs ? EPI_STORE_SPLIT : EPI_STORE16, q, packed ? Bk.qkv.fwg() : Bk.qkv.fw(), s));
  if (ck) dbg_ck(E, st.qkv[l], (size_t)T * 3 * d * 2 * X, s);
  // split operands, some queries only: the other rows of the attention output are not produced, and the backward
  // (delta = rowsum(dO * O) over EVERY row, with dO = 0 off the compact rows) must not meet uninitialised memory there
  if (xs && lr.q_rows > 0 && st.keep) HIPCHK(E, launch_zero(st.attn[l], (size_t)T * d * 2 * X, s));
  if (int rc = attn_fwd(E, st, l, lr.q_rows, false, s)) return rc;
  { ProfScope ps(E, s, PC_GLUE, 0, (double)R * d * 12.0);
    HIPCHK(E, move_rows(st, st.attn[l], c.a16, lr.rows, R, (size_t)d * 2 * X, 0, s));
    if (packed) HIPCHK(E, launch_respk_unpack_rows(st.x[0], (uint8_t*)st.x[0] + (size_t)T * d * 2, st.L, c.x32, R, d, s));
    else HIPCHK(E, move_rows(st, xin, c.x32, lr.rows, R, (size_t)d * 4, 0, s)); }
  if (ck) { dbg_ck(E, c.a16, (size_t)R * d * 2 * X, s); dbg_ck(E, c.x32, (size_t)R * d * 4, s); }
  GemmArgs o = gemm_args(c.a16, R, d, d, c.xm32);
  o.a_split = xs; o.bias = Bk.o.b; o.resid = c.x32;
  HIPCHK(E, gemm(E, EPI_RESID32, o, Bk.o.fw(), s));
  ln = ln_args(c.xm32, Bk.ln2, c.h16, R, d);
  ln.split = xs;
  HIPCHK(E, ln_fwd(E, E->dt, ln, s));
  GemmArgs fc = gemm_args(c.h16, R, 4 * d, d, c.g16);
  fc.a_split = xs; fc.bias = Bk.fc.b;
  if (int rc = mlp_up(E, fc, Bk.fc.fw(), st.keep ? c.u16 : nullptr, c.act32, s)) return rc;
  GemmArgs pr = gemm_args(c.g16, R, d, 4 * d, c.xo32);
  pr.a_split = xs; pr.bias = Bk.pr.b; pr.resid = c.xm32;
  HIPCHK(E, gemm(E, EPI_RESID32, pr, Bk.pr.fw(), s));
  HIPCHK(E, ln_fwd(E, DT_F32, ln_args(c.xo32, lr.ln_close, c.out32, R, d), s));
  return 0;
}
// Backward of last_block_fwd from c.dout32: the closing LayerNorm, MLP, ln_2 and out-proj on the compact rows, the attention backward,
// then the full-width QKV^T GEMM and ln_1 (keys / values of every token).  st.dx32 is zero on entry.  A single-operand tower whose
// forward ran q_rows queries takes the single-query attention backward on the compact rows; every other one scatters the compact dO
// into a zeroed dO16 and runs the attention backward at full width.
int last_block_bwd(Engine* E, const TowerW& W, TowerState& st, Compact& c, const LastRows& lr, hipStream_t s) {
  // (T: the full-width rows that carry a gradient, TowerState::Lg, compact in the gradient buffers)
  const int l = st.layers - 1, T = st.N * st.Lg, R = st.seqs(), d = st.d, xs = st.xs;
  const size_t X = xs ? 2 : 1;
  const Block& Bk = W.blocks[l];
  const bool cls = lr.q_rows > 0 && !xs;
  if (st.saved_rows().seq && (cls || !lr.rows)) return fail(E, MVLPT_ERR_STATE, "last_block_bwd: a gradient length needs the row table of a text tower");
  LnBwdArgs ln = ln_bwd_args(c.dout32, c.xo32, lr.ln_close, c.dx32, R, d);
  ln.out16 = c.dx16; ln.split = xs;
  HIPCHK(E, ln_bwd(E, ln, s));
  GemmArgs up = gemm_args(c.dx16, R, 4 * d, d, c.du16);
  up.a_split = xs; up.aux = c.u16;
  if (int rc = mlp_up_bwd(E, up, Bk.pr.bw(), c.act32, s)) return rc;
  GemmArgs fc = gemm_args(c.du16, R, d, 4 * d, c.dh32);
  fc.a_split = xs;
  HIPCHK(E, gemm(E, EPI_STORE32, fc, Bk.fc.bw(), s));
  ln = ln_bwd_args(c.dh32, c.xm32, Bk.ln2, c.dx32, R, d);
  ln.resid = c.dx32; ln.out16 = c.dx16; ln.split = xs;
  HIPCHK(E, ln_bwd(E, ln, s));
  GemmArgs o = gemm_args(c.dx16, R, d, d, c.dO16);
  o.a_split = xs;
  HIPCHK(E, gemm(E, xs ? EPI_STORE_SPLIT : EPI_STORE16, o, Bk.o.bw(), s));
  { ProfScope ps(E, s, PC_GLUE, 0, (cls ? 0.0 : (double)T * d * 2.0 * X) + (double)R * d * 8.0);
    if (!cls) {
      HIPCHK(E, launch_zero(st.dO16, (size_t)T * d * 2 * X, s));      // (split: dO is a hi|lo pair)
      HIPCHK(E, move_rows(st, c.dO16, st.dO16, lr.rows, R, (size_t)d * 2 * X, 1, s));
    }
    HIPCHK(E, move_rows(st, c.dx32, st.dx32, lr.rows, R, (size_t)d * 4, 1, s)); }     // residual path: d(block input) of the compact rows
  if (int rc = attn_bwd(E, st, l, cls ? &c : nullptr, s)) return rc;
  GemmArgs q = gemm_args(st.dqkv16, T, d, 3 * d, st.dh32);
  q.a_split = xs;
  HIPCHK(E, gemm(E, EPI_STORE32, q, Bk.qkv.bw(), s));
  ln = ln_bwd_args(st.dh32, st.x[2 * l], Bk.ln1, st.dx32, T, d);
  ln.resid = st.dx32; ln.out16 = st.dx16; ln.split = xs; ln.x_rows = st.saved_rows();
  HIPCHK(E, ln_bwd(E, ln, s));
  return 0;
}

// ------------------------------------------------------------------------------------------------ weight loading
bool parse_block_name(const char* rest, int* layer, const char** tail) {
  // rest = "<l>.<tail>"
  char* endp = nullptr;
  long l = strtol(rest, &endp, 10);
  if (endp == rest || *endp != '.') return false;
  *layer = (int)l; *tail = endp + 1; return true;
}

int upload_f32(Engine* E, const float* src32, size_t n, float** dst, hipStream_t s) {
  void* p = nullptr;
  HIPCHK(E, hipMalloc(&p, n * 4));
  E->owned.push_back(p);
  HIPCHK(E, hipMemcpyAsync(p, src32, n * 4, hipMemcpyDeviceToDevice, s));
  *dst = (float*)p; return 0;
}
int pack_linear(Engine* E, const float* w32, int out, int in, Linear* L, hipStream_t s) {
  // rows of [16-bit plane | fp8 plane]: pitch 3K/2 elements (K = the contraction length of that orientation)
  const int ldw = in + in / 2, ldwt = out + out / 2;
  void *w = nullptr, *wt = nullptr;
  HIPCHK(E, hipMalloc(&w, (size_t)out * ldw * 2)); E->owned.push_back(w);
  HIPCHK(E, hipMalloc(&wt, (size_t)in * ldwt * 2)); E->owned.push_back(wt);
  HIPCHK(E, launch_pack_weight(E->dt, w32, w, out, in, ldw, s));
  HIPCHK(E, launch_pack_weight_t(E->dt, w32, wt, out, in, s, ldwt));
  // fp8 planes: W8 = e4m3(W * 2^e8), amax(|W|) * 2^e8 in [128, 256) (e4m3 tops out at 448); the exponent comes back to the
  // host once per tensor (load time), the GEMM gets it by value
  HIPCHK(E, E->ce_ws.reserve(256));
  float* sc = (float*)E->ce_ws.p;
  HIPCHK(E, launch_grad_scale(w32, (size_t)out * in, 128.0f, sc, s));
  HIPCHK(E, launch_pack_weight8(w32, (uint8_t*)w + (size_t)in * 2, out, in, 0, in, (size_t)ldw * 2, sc, s));
  HIPCHK(E, launch_pack_weight8(w32, (uint8_t*)wt + (size_t)out * 2, out, in, 1, out, (size_t)ldwt * 2, sc, s));
  float sc_host = 1.0f;
  HIPCHK(E, hipMemcpyAsync(&sc_host, sc, sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(E, hipStreamSynchronize(s));
  int e8 = 0;
  (void)frexpf(sc_host, &e8);      // sc = 0.5 * 2^e8' -> exponent e8' - 1
  L->w = w; L->wt = wt; L->out = out; L->in = in; L->ldw = ldw; L->ldwt = ldwt; L->e8 = e8 - 1; return 0;
}

// ---- The frozen tensors of a ViT / text handle, each described once: mvlpt_load_frozen, load_block_tensor and first_missing walk
// these lists, the last in list order (the ResNet tower has its own loader, rn_load).  Shape [r], or [r, c] when c != 0.
enum FrozenKind {
  FZ_F32,         // upload_f32 into the float* at `slot`
  FZ_LINEAR,      // pack_linear [r, c] into the Linear at `slot`
  FZ_CONV1,       // visual.conv1.weight [r, 3, c, c]: packed [r, Kp] into the void* at `slot`
  FZ_PROJ,        // visual.proj / text_projection: fp32 in both orientations, into the float* at `slot` and at `slot_t`
  FZ_TOKENS,      // token_embedding.weight [vocab > 0, c]: optional, read by mvlpt_text_encode_tokens only
};
struct FrozenTensor { const char* name; FrozenKind kind; int r, c; void* slot; float** slot_t = nullptr; };
std::vector<FrozenTensor> top_tensors(Engine* E) {
  const MvlptArch& A = E->arch;
  const int dv = A.vision_width, dtw = A.text_width, e = A.embed_dim;
  std::vector<FrozenTensor> v;
  if (!E->rn.on) {
    const int G = A.image_resolution / A.patch_size;
    v = {{"visual.conv1.weight", FZ_CONV1, dv, A.patch_size, &E->conv_w}, {"visual.class_embedding", FZ_F32, dv, 0, &E->cls_emb},
         {"visual.positional_embedding", FZ_F32, G * G + 1, dv, &E->vpos},
         {"visual.ln_pre.weight", FZ_F32, dv, 0, &E->ln_pre.g}, {"visual.ln_pre.bias", FZ_F32, dv, 0, &E->ln_pre.b},
         {"visual.ln_post.weight", FZ_F32, dv, 0, &E->ln_post.g}, {"visual.ln_post.bias", FZ_F32, dv, 0, &E->ln_post.b},
         {"visual.proj", FZ_PROJ, dv, e, &E->vproj, &E->vproj_t}};
  }
  v.insert(v.end(), {{"positional_embedding", FZ_F32, A.context_length, dtw, &E->tpos},
                     {"ln_final.weight", FZ_F32, dtw, 0, &E->ln_final.g}, {"ln_final.bias", FZ_F32, dtw, 0, &E->ln_final.b},
                     {"text_projection", FZ_PROJ, dtw, e, &E->tproj, &E->tproj_t},
                     {"token_embedding.weight", FZ_TOKENS, 0, dtw, &E->tok_emb}});
  return v;
}
// the names behind "resblocks.<l>."
std::array<FrozenTensor, 12> block_tensors(Block& B, int d) {
  return {{{"attn.in_proj_weight", FZ_LINEAR, 3 * d, d, &B.qkv}, {"attn.in_proj_bias", FZ_F32, 3 * d, 0, &B.qkv.b},
           {"attn.out_proj.weight", FZ_LINEAR, d, d, &B.o}, {"attn.out_proj.bias", FZ_F32, d, 0, &B.o.b},
           {"mlp.c_fc.weight", FZ_LINEAR, 4 * d, d, &B.fc}, {"mlp.c_fc.bias", FZ_F32, 4 * d, 0, &B.fc.b},
           {"mlp.c_proj.weight", FZ_LINEAR, d, 4 * d, &B.pr}, {"mlp.c_proj.bias", FZ_F32, d, 0, &B.pr.b},
           {"ln_1.weight", FZ_F32, d, 0, &B.ln1.g}, {"ln_1.bias", FZ_F32, d, 0, &B.ln1.b},
           {"ln_2.weight", FZ_F32, d, 0, &B.ln2.g}, {"ln_2.bias", FZ_F32, d, 0, &B.ln2.b}}};
}
bool frozen_shape_ok(const FrozenTensor& t, const int64_t* shape, int ndim) {
  if (t.kind == FZ_CONV1) return ndim == 4 && shape[0] == t.r && shape[1] == 3 && shape[2] == t.c && shape[3] == t.c;
  if (t.kind == FZ_TOKENS) return ndim == 2 && shape[0] > 0 && shape[0] <= INT32_MAX && shape[1] == t.c;
  return t.c ? (ndim == 2 && shape[0] == t.r && shape[1] == t.c) : (ndim == 1 && shape[0] == t.r);
}
const void* frozen_loaded(const FrozenTensor& t) {
  return t.kind == FZ_LINEAR ? ((const Linear*)t.slot)->w : t.kind == FZ_CONV1 ? *(void**)t.slot : *(float**)t.slot;
}
// `p`: the tensor as fp32 on the device, of a shape frozen_shape_ok has accepted
int frozen_load(Engine* E, const FrozenTensor& t, const float* p, const int64_t* shape, hipStream_t s) {
  const size_t n = (size_t)t.r * (t.c ? t.c : 1);
  switch (t.kind) {
    case FZ_F32: return upload_f32(E, p, n, (float**)t.slot, s);
    case FZ_LINEAR: return pack_linear(E, p, t.r, t.c, (Linear*)t.slot, s);
    case FZ_CONV1: {
      void* w = nullptr;
      HIPCHK(E, hipMalloc(&w, (size_t)t.r * E->Kp * 2)); E->owned.push_back(w);
      HIPCHK(E, launch_pack_weight(E->dt, p, w, t.r, 3 * t.c * t.c, E->Kp, s));
      *(void**)t.slot = w;
      return 0;
    }
    case FZ_PROJ: {
      // proj is [r, c]: forward Bt = proj^T [c, r]; dX Bt = proj [r, c]; both kept in fp32 (the projections next to the logits)
      void *w = nullptr, *wt = nullptr;
      HIPCHK(E, hipMalloc(&w, n * 4)); E->owned.push_back(w);
      HIPCHK(E, hipMalloc(&wt, n * 4)); E->owned.push_back(wt);
      HIPCHK(E, launch_pack_weight(DT_F32, p, w, t.r, t.c, t.c, s));
      HIPCHK(E, launch_pack_weight_t(DT_F32, p, wt, t.r, t.c, s));
      *(float**)t.slot = (float*)w; *t.slot_t = (float*)wt;
      return 0;
    }
    case FZ_TOKENS: {
      E->vocab = 0;
      const int rc = upload_f32(E, p, (size_t)shape[0] * t.c, (float**)t.slot, s);
      if (!rc) E->vocab = (int)shape[0];
      return rc;
    }
  }
  return 0;
}

int load_block_tensor(Engine* E, TowerW& W, int layer, const char* tail, const float* p, const int64_t* shape, int ndim,
                      hipStream_t s) {
  if (layer < 0 || layer >= W.layers) return fail(E, MVLPT_ERR_ARG, "layer index out of range");
  for (const FrozenTensor& t : block_tensors(W.blocks[layer], W.width)) {
    if (strcmp(tail, t.name)) continue;
    if (!frozen_shape_ok(t, shape, ndim)) return fail(E, MVLPT_ERR_ARG, std::string("shape mismatch for block tensor ") + tail);
    return frozen_load(E, t, p, shape, s);
  }
  return fail(E, MVLPT_ERR_ARG, std::string("unknown block tensor: ") + tail);
}

const char* first_missing(Engine* E) {
  static thread_local std::string m;
  auto chk = [&](const void* p, const std::string& n) { if (!p && m.empty()) m = n; };
  m.clear();
  if (E->rn.on) {
    auto conv = [&](const ConvW& c, const std::string& cn, const std::string& bn) {
      chk(c.w, cn + ".weight"); chk(c.bn.g, bn + ".weight"); chk(c.bn.b, bn + ".bias");
      chk(c.bn.m, bn + ".running_mean"); chk(c.bn.v, bn + ".running_var");
    };
    for (int i = 0; i < 3; ++i) conv(E->rn.stem[i], "visual.conv" + std::to_string(i + 1), "visual.bn" + std::to_string(i + 1));
    for (int st = 0; st < 4; ++st)
      for (size_t i = 0; i < E->rn.stage[st].size(); ++i) {
        const RNBlock& B = E->rn.stage[st][i];
        const std::string q = "visual.layer" + std::to_string(st + 1) + "." + std::to_string(i) + ".";
        conv(B.c1, q + "conv1", q + "bn1"); conv(B.c2, q + "conv2", q + "bn2"); conv(B.c3, q + "conv3", q + "bn3");
        if (B.has_ds) conv(B.ds, q + "downsample.0", q + "downsample.1");
      }
    chk(E->rn.pos, "visual.attnpool.positional_embedding");
    static const char* const pn[4] = {"q", "k", "v", "c"};
    for (int i = 0; i < 4; ++i) {
      if (!E->rn.have[i] && m.empty()) m = std::string("visual.attnpool.") + pn[i] + "_proj.weight";
      if (!E->rn.have[4 + i] && m.empty()) m = std::string("visual.attnpool.") + pn[i] + "_proj.bias";
    }
  }
  // (every forward asks: a name is put together only for a tensor that is missing)
  for (const FrozenTensor& t : top_tensors(E)) if (t.kind != FZ_TOKENS && !frozen_loaded(t) && m.empty()) m = t.name;
  for (int t = 0; t < 2; ++t) {
    TowerW& W = t ? E->txt : E->vis;
    for (int l = 0; l < W.layers; ++l)
      for (const FrozenTensor& b : block_tensors(W.blocks[l], W.width))
        if (!frozen_loaded(b) && m.empty()) m = (t ? "transformer.resblocks." : "visual.transformer.resblocks.") + std::to_string(l) + "." + b.name;
  }
  return m.empty() ? nullptr : m.c_str();
}

// LayerNorm folding: the per-column vectors of every linear layer that follows a LayerNorm (qkv <- ln_1, fc <- ln_2), once,
// when all frozen tensors are there (the first tower forward)
int prepare_fold(Engine* E, hipStream_t s) {
  if (E->fold_ready) return 0;
  // A REBUILD (frozen tensors reloaded, packed stream toggled) rewrites vectors the other tower — on another stream — may still be
  // reading: drain the device first.  Rare and outside any step; the first build has no readers.
  if (!E->vis.blocks.empty() && E->vis.blocks[0].qkv.fold_s) HIPCHK(E, hipDeviceSynchronize());
  for (TowerW* W : {&E->vis, &E->txt}) {
    const int d = W->width;
    for (Block& B : W->blocks) {
      for (int k = 0; k < 2; ++k) {
        Linear& L = k ? B.fc : B.qkv;
        const LNp& ln = k ? B.ln2 : B.ln1;
        if (!L.fold_s) {      // (kept across reloads of the frozen tensors: the shapes are fixed by the architecture)
          void* p = nullptr;
          HIPCHK(E, hipMalloc(&p, (size_t)L.out * 2 * sizeof(float)));
          E->owned.push_back(p);
          L.fold_s = (float*)p; L.fold_b = (float*)p + L.out;
        }
        HIPCHK(E, launch_fold_vectors(E->dt, L.w, L.ldw, ln.g, ln.b, L.b, L.fold_s, L.fold_b, L.out, d, s));
        if (W == &E->vis && E->dt == DT_F16 && E->resid_packed) {      // packed residual stream: gamma inside the weight
          if (!L.wg) {
            void* p = nullptr;
            HIPCHK(E, hipMalloc(&p, (size_t)L.out * L.in * 2 + (size_t)L.out * sizeof(float)));
            E->owned.push_back(p);
            L.wg = p; L.fold_sg = (float*)((char*)p + (size_t)L.out * L.in * 2);
          }
          HIPCHK(E, launch_fold_weight(L.w, L.ldw, ln.g, L.wg, L.in, L.fold_sg, L.out, d, s));
        }
      }
    }
  }
  // Both towers' vectors are computed on the stream of whichever tower gets here first; the other tower runs on another
  // stream and reads them without any dependency on `s`.  One host-side wait, once per (re)load of the frozen tensors.
  HIPCHK(E, hipStreamSynchronize(s));
  E->fold_ready = true;
  return 0;
}

// A ViT image tower whose heads are wider than 64 (ViT-H/14: 16 heads of 80) has the forward kernel of attention_wide.hip and nothing else
const char* kRefuseWide = "an image tower with heads wider than 64 is frozen, prompt-free and forward-only on single 16-bit operands: ";
static bool vision_wide(const Engine* E) { return !E->rn.on && E->vis.heads > 0 && E->vis.width != E->vis.heads * 64; }

// ------------------------------------------------------------------------------------------------ ModifiedResNet image tower
const char* kRefuseRN = "the ResNet image tower is frozen and forward-only in one piece (trainers/mvlpt.py:48 cannot prompt a ResNet): ";

int rn_load_conv(Engine* E, ConvW& c, const float* p, const int64_t* shape, int ndim, const std::string& nm, hipStream_t s) {
  if (!(ndim == 4 && shape[0] == c.cout && shape[1] == c.cin && shape[2] == c.k && shape[3] == c.k))
    return fail(E, MVLPT_ERR_ARG, "shape mismatch: " + nm);
  if (!c.w) {
    void* w = nullptr;
    HIPCHK(E, hipMalloc(&w, (size_t)c.cout * conv_kp(c.k, c.cin_pad) * 2)); E->owned.push_back(w);
    c.w = w;
  }
  HIPCHK(E, launch_pack_conv_weight(p, c.w, c.cout, c.cin, c.k, c.cin_pad, s));
  return 0;
}
int rn_load_bn(Engine* E, ConvW& c, const std::string& field, const float* p, const int64_t* shape, int ndim, const std::string& nm,
               hipStream_t s) {
  if (!(ndim == 1 && shape[0] == c.cout)) return fail(E, MVLPT_ERR_ARG, "shape mismatch: " + nm);
  float** dst = field == "weight" ? &c.bn.g : field == "bias" ? &c.bn.b : field == "running_mean" ? &c.bn.m
                : field == "running_var" ? &c.bn.v : nullptr;
  if (!dst) return fail(E, MVLPT_ERR_ARG, "unknown frozen tensor name: " + nm);
  return upload_f32(E, p, (size_t)c.cout, dst, s);
}
// "<conv>.weight" / "<bn>.<field>" of one conv + BatchNorm pair; `t` is the name behind the pair's prefix
int rn_load_pair(Engine* E, ConvW& c, const std::string& t, const std::string& conv, const std::string& bn, const float* p,
                 const int64_t* shape, int ndim, const std::string& nm, hipStream_t s) {
  if (t == conv + ".weight") return rn_load_conv(E, c, p, shape, ndim, nm, s);
  if (t.rfind(bn + ".", 0) == 0) return rn_load_bn(E, c, t.substr(bn.size() + 1), p, shape, ndim, nm, s);
  return 1;      // not this pair
}

int rn_load(Engine* E, const std::string& nm, const float* p, const int64_t* shape, int ndim, hipStream_t s) {
  ResNetW& R = E->rn;
  R.ready = false;
  const std::string t = nm.substr(7);      // behind "visual."
  const int Ech = 32 * R.a.width, T = (R.a.image_resolution / 32) * (R.a.image_resolution / 32) + 1;
  for (int i = 0; i < 3; ++i) {
    const int rc = rn_load_pair(E, R.stem[i], t, "conv" + std::to_string(i + 1), "bn" + std::to_string(i + 1), p, shape, ndim, nm, s);
    if (rc <= 0) return rc;
  }
  if (t.rfind("layer", 0) == 0 && t.size() > 7 && t[5] >= '1' && t[5] <= '4' && t[6] == '.') {
    const int st = t[5] - '1';
    char* endp = nullptr;
    const long bi = strtol(t.c_str() + 7, &endp, 10);
    if (endp == t.c_str() + 7 || *endp != '.' || bi < 0 || bi >= (long)R.stage[st].size())
      return fail(E, MVLPT_ERR_ARG, "block index out of range: " + nm);
    RNBlock& B = R.stage[st][bi];
    const std::string u(endp + 1);
    int rc = rn_load_pair(E, B.c1, u, "conv1", "bn1", p, shape, ndim, nm, s); if (rc <= 0) return rc;
    rc = rn_load_pair(E, B.c2, u, "conv2", "bn2", p, shape, ndim, nm, s); if (rc <= 0) return rc;
    rc = rn_load_pair(E, B.c3, u, "conv3", "bn3", p, shape, ndim, nm, s); if (rc <= 0) return rc;
    if (B.has_ds) { rc = rn_load_pair(E, B.ds, u, "downsample.0", "downsample.1", p, shape, ndim, nm, s); if (rc <= 0) return rc; }
    return fail(E, MVLPT_ERR_ARG, "unknown frozen tensor name: " + nm);
  }
  if (t == "attnpool.positional_embedding") {
    if (!(ndim == 2 && shape[0] == T && shape[1] == Ech)) return fail(E, MVLPT_ERR_ARG, "shape mismatch: " + nm);
    return upload_f32(E, p, (size_t)T * Ech, &R.pos, s);
  }
  static const char* const pn[4] = {"q", "k", "v", "c"};
  for (int i = 0; i < 4; ++i) {
    const std::string base = std::string("attnpool.") + pn[i] + "_proj.";
    const int out = i == 3 ? R.a.output_dim : Ech;
    if (t == base + "weight") {
      if (!(ndim == 2 && shape[0] == out && shape[1] == Ech)) return fail(E, MVLPT_ERR_ARG, "shape mismatch: " + nm);
      void** w = i == 0 ? &R.qw : i == 3 ? &R.cw : &R.kvw;
      if (!*w) {
        void* q = nullptr;
        HIPCHK(E, hipMalloc(&q, (size_t)(i == 1 || i == 2 ? 2 : 1) * out * Ech * 2)); E->owned.push_back(q);
        *w = q;
      }
      HIPCHK(E, launch_pack_weight(DT_F16, p, (char*)*w + (i == 2 ? (size_t)Ech * Ech * 2 : 0), out, Ech, Ech, s));
      R.have[i] = true;
      return 0;
    }
    if (t == base + "bias") {
      if (!(ndim == 1 && shape[0] == out)) return fail(E, MVLPT_ERR_ARG, "shape mismatch: " + nm);
      float** b = i == 0 ? &R.qb : i == 3 ? &R.cb : &R.kvb;
      if (!*b) {
        void* q = nullptr;
        HIPCHK(E, hipMalloc(&q, (size_t)(i == 1 || i == 2 ? 2 : 1) * out * 4)); E->owned.push_back(q);
        *b = (float*)q;
      }
      HIPCHK(E, hipMemcpyAsync(*b + (i == 2 ? Ech : 0), p, (size_t)out * 4, hipMemcpyDeviceToDevice, s));
      R.have[4 + i] = true;
      return 0;
    }
  }
  return fail(E, MVLPT_ERR_ARG, "unknown frozen tensor name: " + nm);
}

// BatchNorm scale / shift of every conv, once behind a (re)load of the frozen tensors
int prepare_resnet(Engine* E, hipStream_t s) {
  ResNetW& R = E->rn;
  if (R.ready) return 0;
  int rc = 0;
  auto one = [&](ConvW& c) {
    if (rc) return;
    if (!c.bn.scale) {
      void* p = nullptr;
      hipError_t e = hipMalloc(&p, (size_t)c.cout * 2 * sizeof(float));
      if (e != hipSuccess) { rc = hipfail(E, e, "hipMalloc"); return; }
      E->owned.push_back(p);
      c.bn.scale = (float*)p; c.bn.shift = (float*)p + c.cout;
    }
    hipError_t e = launch_bn_affine(c.bn.g, c.bn.b, c.bn.m, c.bn.v, 1e-5f, c.bn.scale, c.bn.shift, c.cout, s);
    if (e != hipSuccess) rc = hipfail(E, e, "launch_bn_affine");
  };
  if (R.stem[0].bn.scale) HIPCHK(E, hipDeviceSynchronize());      // a rebuild: another stream may still read the old vectors
  for (ConvW& c : R.stem) one(c);
  for (auto& st : R.stage) for (RNBlock& B : st) { one(B.c1); one(B.c2); one(B.c3); if (B.has_ds) one(B.ds); }
  if (rc) return rc;
  HIPCHK(E, hipStreamSynchronize(s));      // (the next forward may run on another stream)
  R.ready = true;
  return 0;
}

// conv + BatchNorm + ReLU of one ConvW at stride 1, no residual: what most of the tower's convolutions are
ConvArgs conv_args(const ConvW& c, const void* x, void* y, int B, int H, int W) {
  return ConvArgs{x, c.w, c.bn.scale, c.bn.shift, nullptr, y, B, H, W, c.cin_pad, c.cout, c.k, 1, 1};
}

int resnet_fwd(Engine* E, const void* image, int image_dtype, int B, float* feat_out, hipStream_t s) {
  ResNetW& R = E->rn;
  if (int rc = prepare_resnet(E, s)) return rc;
  const int res = R.a.image_resolution, w = R.a.width, g = res / 32, HW = g * g, T = HW + 1, Ech = 32 * w, e = R.a.output_dim;
  if ((size_t)B * res * res / 4 * w > (size_t)1 << 40 || B > 65535) return fail(E, MVLPT_ERR_ARG, "image_fwd: batch too large");
  // the largest map: the stem's last conv and the first stage's output, B * (res/2)^2 * w elements; five maps live at once
  const size_t mapn = (size_t)B * (res / 2) * (res / 2) * w;
  E->vrun = ImageRun();      // opened: the workspace below no longer holds the last transformer forward
  void *img8, *buf[5], *tok, *kv, *q16, *o16;
  if (int rc = carve_ws(E, E->vis_ws, "image_fwd (ResNet)", kCarveSlack, [&](Bump& bp) {
        img8 = bp.take_bytes((size_t)B * res * res * 8 * 2);
        for (void*& b : buf) b = bp.take_bytes(mapn * 2);
        tok = bp.take_bytes((size_t)B * T * Ech * 2);
        kv = bp.take_bytes((size_t)B * T * 2 * Ech * 2);
        q16 = bp.take_bytes((size_t)B * Ech * 2);
        o16 = bp.take_bytes((size_t)B * Ech * 2);
      })) return rc;
  void *x = buf[0], *a = buf[1], *b = buf[2], *c = buf[3], *d = buf[4];

  { ProfScope ps(E, s, PC_GLUE, 0, (double)B * res * res * (3.0 * 4.0 + 16.0));
    HIPCHK(E, launch_nchw_to_nhwc8(image, image_dtype, img8, B, res, s)); }
  int H = res / 2;      // the stem: conv3x3 stride 2, conv3x3, conv3x3 (each + BN + ReLU), AvgPool2d(2)
  ConvArgs stem0 = conv_args(R.stem[0], img8, a, B, res, res);
  stem0.stride = 2;
  HIPCHK(E, launch_conv2d(stem0, s));
  HIPCHK(E, launch_conv2d(conv_args(R.stem[1], a, b, B, H, H), s));
  HIPCHK(E, launch_conv2d(conv_args(R.stem[2], b, a, B, H, H), s));
  HIPCHK(E, launch_avgpool2x2(a, x, B, H, H, w, s));
  H /= 2;
  for (int st = 0; st < 4; ++st)
    for (const RNBlock& K : R.stage[st]) {
      // Bottleneck (clip/model.py:10-55): every strided convolution is an average pool in front of a stride-1 convolution
      const int Ho = H / K.stride;
      HIPCHK(E, launch_conv2d(conv_args(K.c1, x, a, B, H, H), s));
      HIPCHK(E, launch_conv2d(conv_args(K.c2, a, b, B, H, H), s));
      const void* main_in = b;
      if (K.stride > 1) { HIPCHK(E, launch_avgpool2x2(b, a, B, H, H, K.c2.cout, s)); main_in = a; }
      const void* identity = x;
      if (K.has_ds) {
        const void* ds_in = x;
        if (K.stride > 1) { HIPCHK(E, launch_avgpool2x2(x, c, B, H, H, K.ds.cin, s)); ds_in = c; }
        ConvArgs ds = conv_args(K.ds, ds_in, d, B, Ho, Ho);
        ds.relu = 0;
        HIPCHK(E, launch_conv2d(ds, s));
        identity = d;
      }
      void* out = b == main_in ? a : b;
      ConvArgs c3 = conv_args(K.c3, main_in, out, B, Ho, Ho);
      c3.resid = identity;
      HIPCHK(E, launch_conv2d(c3, s));
      if (out == a) { a = x; x = out; } else { b = x; x = out; }
      H = Ho;
    }
  // AttentionPool2d (clip/model.py:58-91): only token 0's output is returned, so only its query is projected
  { ProfScope ps(E, s, PC_GLUE, 0, (double)B * T * Ech * 4.0);
    HIPCHK(E, launch_attnpool_tokens(x, R.pos, tok, B, HW, Ech, s)); }
  GemmArgs gq = gemm_args(tok, B, Ech, Ech, q16);      // (row b: token 0 of image b)
  gq.bias = R.qb; gq.lda = T * Ech;
  HIPCHK(E, gemm(E, EPI_STORE16, gq, WRef{R.qw, Ech, 0}, s, DT_F16));
  GemmArgs gkv = gemm_args(tok, B * T, 2 * Ech, Ech, kv);
  gkv.bias = R.kvb;
  HIPCHK(E, gemm(E, EPI_STORE16, gkv, WRef{R.kvw, Ech, 0}, s, DT_F16));
  { ProfScope ps(E, s, PC_ATTN_FWD, 4.0 * T * 64.0 * B * (Ech / 64), (double)B * T * 2 * Ech * 2.0);
    HIPCHK(E, launch_attnpool_query(q16, kv, o16, B, T, Ech, s)); }
  GemmArgs gc = gemm_args(o16, B, e, Ech, feat_out);
  gc.bias = R.cb;
  HIPCHK(E, gemm(E, EPI_STORE32, gc, WRef{R.cw, Ech, 0}, s, DT_F16));
  E->vrun.phase = Phase::Done;
  return 0;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" {

#ifndef MVLPT_SRC_HASH
#define MVLPT_SRC_HASH "unknown"
#endif
#ifndef MVLPT_GIT_HASH
#define MVLPT_GIT_HASH "nogit"
#endif
// "mvlpt_hip 0.1 (gfx950) src:<sha256 of csrc/*.hip csrc/*.h include/mvlpt_hip.h, 12 hex> git:<commit the tree was built in>"
const char* mvlpt_version(void) { return "mvlpt_hip 0.1 (gfx950) src:" MVLPT_SRC_HASH " git:" MVLPT_GIT_HASH; }

const char* mvlpt_last_error(void* h) { return h ? ((Engine*)h)->err.c_str() : g_create_err.c_str(); }

// What mvlpt_create and mvlpt_create_resnet share.  arch_check: the transformer limits, in the order both entries report them.
// vit = false (create_resnet): the ViT vision fields are 0, as that entry has checked, and put nothing in the way of the text tower's checks.
static int arch_check(const MvlptArch* a, bool vit) {
  // the text tower's heads are 64 wide; a ViT image tower's may be 80 / 96 / 112 / 128 as well (vision_wide)
  bool vis_ok = a->vision_width == a->vision_heads * 64;
  if (vit && !vis_ok && a->vision_heads > 0 && a->vision_width % a->vision_heads == 0) vis_ok = attn_wide_supported(a->vision_width / a->vision_heads);
  if (!vis_ok || a->text_width != a->text_heads * 64)
    return fail(nullptr, MVLPT_ERR_UNSUPPORTED, vit ? "head_dim must be 64 (CLIP ViT: heads = width // 64), or 80 / 96 / 112 / 128 in the image tower" : "head_dim must be 64");
  if (a->vision_width % 128 || a->text_width % 128 || a->embed_dim % 64)
    return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "widths must be multiples of 128 and embed_dim of 64");
  if (vit && (a->patch_size <= 0 || a->image_resolution % a->patch_size))
    return fail(nullptr, MVLPT_ERR_ARG, "image_resolution must be a multiple of patch_size");
  if ((vit && a->vision_layers <= 0) || a->text_layers <= 0 || a->context_length <= 0)
    return fail(nullptr, MVLPT_ERR_ARG, "bad layer count / context length");
  return 0;
}
// engine_new: the device probe, a handle with the environment's overrides and the text tower sized.  The ResNet tower has no packed
// stream: its entry does not read MVLPT_RESID_PACKED.
static int engine_new(const MvlptArch* a, bool read_resid_packed, Engine** out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, MVLPT_ERR_HIP, "no HIP device visible: libmvlpt_hip needs an AMD GPU (there is no CPU fallback)");
  Engine* E = new Engine();
  E->arch = *a; E->dt = a->compute_dtype;
  if (const char* v = getenv("MVLPT_SPLIT_LO8")) E->lo8 = atoi(v) != 0;
  if (const char* v = getenv("MVLPT_LN_FOLD")) E->fold_mode = atoi(v);
  if (const char* v = read_resid_packed ? getenv("MVLPT_RESID_PACKED") : nullptr) E->resid_packed = atoi(v) ? 1 : 0;
  if (const char* v = getenv("MVLPT_LN_FOLD_MIN_ROWS")) E->fold_min_rows = atoi(v) > 0 ? atoi(v) : 1;
  E->txt.width = a->text_width; E->txt.layers = a->text_layers; E->txt.heads = a->text_heads;
  E->txt.blocks.resize(a->text_layers);
  *out = E;
  return 0;
}

int mvlpt_create(const MvlptArch* a, void** handle) {
  if (!a || !handle) return fail(nullptr, MVLPT_ERR_ARG, "null argument");
  if (a->compute_dtype != MVLPT_DT_F16 && a->compute_dtype != MVLPT_DT_BF16)
    return fail(nullptr, MVLPT_ERR_ARG, "compute_dtype must be MVLPT_DT_F16 or MVLPT_DT_BF16");
  if (int rc = arch_check(a, true)) return rc;
  Engine* E = nullptr;
  if (int rc = engine_new(a, true, &E)) return rc;
  E->vis.width = a->vision_width; E->vis.layers = a->vision_layers; E->vis.heads = a->vision_heads;
  E->vis.blocks.resize(a->vision_layers);
  const int K = 3 * a->patch_size * a->patch_size;
  E->Kp = (K + 63) / 64 * 64;
  *handle = E;
  return 0;
}

int mvlpt_create_resnet(const MvlptArch* a, const MvlptResNetArch* rn, void** handle) {
  if (!a || !rn || !handle) return fail(nullptr, MVLPT_ERR_ARG, "null argument");
  if (a->image_resolution || a->patch_size || a->vision_width || a->vision_layers || a->vision_heads)
    return fail(nullptr, MVLPT_ERR_ARG, "create_resnet: the ViT vision fields of MvlptArch must be 0");
  if (a->compute_dtype == MVLPT_DT_BF16) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "create_resnet: the ResNet tower computes in fp16 only");
  if (a->compute_dtype != MVLPT_DT_F16) return fail(nullptr, MVLPT_ERR_ARG, "compute_dtype must be MVLPT_DT_F16");
  if (int rc = arch_check(a, false)) return rc;
  if (rn->image_resolution <= 0 || rn->image_resolution % 32) return fail(nullptr, MVLPT_ERR_ARG, "create_resnet: image_resolution must be a positive multiple of 32");
  if (rn->width <= 0 || rn->width % 4) return fail(nullptr, MVLPT_ERR_ARG, "create_resnet: width must be a positive multiple of 4");
  for (int i = 0; i < 4; ++i) if (rn->layers[i] <= 0) return fail(nullptr, MVLPT_ERR_ARG, "create_resnet: every stage needs at least one block");
  if (rn->heads * 64 != 32 * rn->width) return fail(nullptr, MVLPT_ERR_ARG, "create_resnet: heads * 64 must equal 32 * width");
  if (rn->output_dim != a->embed_dim) return fail(nullptr, MVLPT_ERR_ARG, "create_resnet: output_dim must equal embed_dim");
  if (rn->width % 16 || rn->output_dim % 128)      // stem channels width / 2 in runs of 8; the projections run on the 128-column GEMM tiles
    return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "create_resnet: width must be a multiple of 16 and output_dim of 128");
  const int g = rn->image_resolution / 32;
  if (g * g + 1 > attnpool_max_tokens()) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "create_resnet: more than 145 attention-pool tokens");
  Engine* E = nullptr;
  if (int rc = engine_new(a, false, &E)) return rc;
  ResNetW& R = E->rn;
  R.on = true; R.a = *rn;
  const int w = rn->width;
  auto conv = [](ConvW& c, int cin, int cout, int k) { c.cin = cin; c.cin_pad = (cin + 7) / 8 * 8; c.cout = cout; c.k = k; };
  conv(R.stem[0], 3, w / 2, 3); conv(R.stem[1], w / 2, w / 2, 3); conv(R.stem[2], w / 2, w, 3);
  int inplanes = w;
  for (int st = 0; st < 4; ++st) {
    const int planes = w << st;
    R.stage[st].resize(rn->layers[st]);
    for (int i = 0; i < rn->layers[st]; ++i) {
      RNBlock& B = R.stage[st][i];
      B.stride = (i == 0 && st > 0) ? 2 : 1;
      B.has_ds = B.stride > 1 || inplanes != planes * 4;
      conv(B.c1, inplanes, planes, 1); conv(B.c2, planes, planes, 3); conv(B.c3, planes, planes * 4, 1);
      if (B.has_ds) conv(B.ds, inplanes, planes * 4, 1);
      inplanes = planes * 4;
    }
  }
  *handle = E;
  return 0;
}

int mvlpt_set_precision(void* h, int mode) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  if (mode != MVLPT_PREC_FAST && mode != MVLPT_PREC_SPLIT_GRAD && mode != MVLPT_PREC_SPLIT_ALL)
    return fail(E, MVLPT_ERR_ARG, "set_precision: unknown mode");
  E->prec_mode = mode;
  return 0;
}

int mvlpt_set_activation(void* h, int act) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  if (act != MVLPT_ACT_QUICKGELU && act != MVLPT_ACT_GELU)
    return fail(E, MVLPT_ERR_ARG, "set_activation: the activation is MVLPT_ACT_QUICKGELU or MVLPT_ACT_GELU");
  // a saved state was carved for, and its pre-activations belong to, the activation of its forward: the backward must see the same
  if (E->vrun.phase == Phase::Pending || E->vrun.phase == Phase::Saved || E->trun.phase == Phase::Saved)
    return fail(E, MVLPT_ERR_STATE, "set_activation: a forward has saved activations whose backward has not run (or an image forward is "
                                    "pending); change the activation before a forward or after a completed step");
  E->act = act;
  return 0;
}
int mvlpt_get_activation(void* h, int* act) {
  Engine* E = (Engine*)h;
  if (!E || !act) return fail(E, MVLPT_ERR_ARG, "get_activation: null argument");
  *act = E->act;
  return 0;
}

int mvlpt_stream_create_cus(int cu_first, int cu_count, mvlpt_stream_t* stream) {
  if (!stream) return fail(nullptr, MVLPT_ERR_ARG, "stream_create_cus: null argument");
  const int total = device_cus();
  if (cu_first < 0 || cu_count <= 0 || cu_first + cu_count > total)
    return fail(nullptr, MVLPT_ERR_ARG, "stream_create_cus: CU range outside the device (" + std::to_string(total) + " compute units)");
  // bit i of the mask = logical compute unit i; the driver deals logical CUs round-robin over the XCDs (bit i -> XCD i % 8),
  // so a contiguous range of 8k bits is k compute units on EVERY XCD: each partition keeps all eight L2s
  std::vector<uint32_t> mask((total + 31) / 32, 0u);
  for (int i = cu_first; i < cu_first + cu_count; ++i) mask[i >> 5] |= 1u << (i & 31);
  hipStream_t s = nullptr;
  hipError_t e = hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data());
  if (e != hipSuccess) return hipfail(nullptr, e, "hipExtStreamCreateWithCUMask");
  { std::lock_guard<std::mutex> lk(g_part_mu); g_parts.push_back(StreamPart{s, cu_count}); }
  *stream = (mvlpt_stream_t)s;
  return 0;
}

int mvlpt_stream_destroy(mvlpt_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!s) return 0;
  {
    std::lock_guard<std::mutex> lk(g_part_mu);
    for (size_t i = 0; i < g_parts.size(); ++i) if (g_parts[i].s == s) { g_parts.erase(g_parts.begin() + i); break; }
    for (size_t i = 0; i < g_caps.size(); ++i) if (g_caps[i].s == s) { g_caps.erase(g_caps.begin() + i); break; }
  }
  hipError_t e = hipStreamDestroy(s);
  if (e != hipSuccess) return hipfail(nullptr, e, "hipStreamDestroy");
  return 0;
}

int mvlpt_stream_cus(mvlpt_stream_t stream) { return stream_cus((hipStream_t)stream); }

int mvlpt_stream_set_cu_cap(mvlpt_stream_t stream, int n) {
  hipStream_t s = (hipStream_t)stream;
  if (!s) return fail(nullptr, MVLPT_ERR_ARG, "stream_set_cu_cap: the NULL stream cannot be capped");
  if (n > 0 && n < 8) return fail(nullptr, MVLPT_ERR_ARG, "stream_set_cu_cap: a cap is at least 8 compute units (one per XCD)");
  const int cap = n > 0 ? n / 8 * 8 : 0;      // workgroup b runs on XCD b % 8: the same share of every XCD
  std::lock_guard<std::mutex> lk(g_part_mu);
  for (size_t i = 0; i < g_caps.size(); ++i)
    if (g_caps[i].s == s) {
      if (cap > 0) g_caps[i].cus = cap; else g_caps.erase(g_caps.begin() + i);
      return 0;
    }
  if (cap > 0) g_caps.push_back(StreamPart{s, cap});
  return 0;
}

int mvlpt_set_resid_packed(void* h, int on) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  if ((on != 0) != (E->resid_packed != 0)) E->fold_ready = false;      // the gamma-folded weights are built by prepare_fold
  E->resid_packed = on ? 1 : 0;
  return 0;
}
int mvlpt_set_ln_fold(void* h, int mode, int min_rows) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  if (mode < 0 || mode > 2 || min_rows < 1) return fail(E, MVLPT_ERR_ARG, "set_ln_fold: mode in {0, 1, 2}, min_rows >= 1");
  E->fold_mode = mode; E->fold_min_rows = min_rows;
  return 0;
}

int mvlpt_set_vpt_dropout(void* h, const float* masks, int n_layers, int batch, int n_vpt, int width) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  if (E->rn.on) return fail(E, MVLPT_ERR_UNSUPPORTED, std::string(kRefuseRN) + "set_vpt_dropout");
  if (vision_wide(E)) return fail(E, MVLPT_ERR_UNSUPPORTED, std::string(kRefuseWide) + "set_vpt_dropout");
  if (masks && (n_layers <= 0 || batch <= 0 || n_vpt <= 0 || width != E->arch.vision_width))
    return fail(E, MVLPT_ERR_ARG, "set_vpt_dropout: masks are [n_layers, batch, n_vpt, vision_width], every extent positive");
  E->vpt_mask = masks ? Engine::VptMask{masks, n_layers, batch, n_vpt} : Engine::VptMask{};
  return 0;
}

int mvlpt_debug_checksums(void* h, int enable, unsigned long long* host_out, int max_out) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  int n = 0;
  if (host_out && max_out > 0 && E->dbg_ck) {
    HIPCHK(E, hipDeviceSynchronize());
    n = E->dbg_ck_n < max_out ? E->dbg_ck_n : max_out;
    HIPCHK(E, hipMemcpy(host_out, E->dbg_ck, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }
  if (enable && !E->dbg_ck) {
    void* p = nullptr;
    HIPCHK(E, hipMalloc(&p, DBG_CK_MAX * sizeof(unsigned long long)));
    E->owned.push_back(p);
    E->dbg_ck = (unsigned long long*)p;
  }
  E->dbg_ck_on = enable != 0;
  return n;
}

int mvlpt_trim(void* h) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  HIPCHK(E, hipDeviceSynchronize());       // epoch boundary: a host-side pause is acceptable here, never inside a step
  for (DevBuf* b : {&E->vis_ws, &E->txt_ws, &E->head_ws, &E->ce_ws, &E->tmp, &E->pp_ws, &E->near_ws}) (void)b->trim();
  return 0;
}

int mvlpt_destroy(void* h) {
  if (!h) return 0;
  Engine* E = (Engine*)h;
  (void)hipDeviceSynchronize();
  for (void* p : E->owned) (void)hipFree(p);
  for (hipEvent_t ev : E->ev_pool) (void)hipEventDestroy(ev);
  delete E;
  return 0;
}

int mvlpt_load_frozen(void* h, const char* name, const void* dev_ptr, int dtype, const int64_t* shape, int ndim,
                      mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !name || !dev_ptr || !shape || ndim < 0 || ndim > 4) return fail(E, MVLPT_ERR_ARG, "null/invalid argument");
  hipStream_t s = (hipStream_t)stream;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  std::string nm(name);
  if (nm == "logit_scale") return 0;  // not used by the towers
  const std::vector<FrozenTensor> tops = top_tensors(E);
  const FrozenTensor* top = nullptr;
  for (const FrozenTensor& t : tops) if (nm == t.name) top = &t;
  // the token table is read by mvlpt_text_encode_tokens only: the towers' packed state is untouched.  Every other call, a refused one
  // too: W gamma / b + W beta of the LayerNorm folding are rebuilt from the new tensors (prepare_fold)
  if (!(top && top->kind == FZ_TOKENS)) E->fold_ready = false;
  // stage as fp32
  const float* p32 = (const float*)dev_ptr;
  if (dtype != MVLPT_DT_F32) {
    HIPCHK(E, E->tmp.reserve(n * 4));
    HIPCHK(E, launch_cast_any_to_f32(dtype, dev_ptr, (float*)E->tmp.p, n, s));
    p32 = (const float*)E->tmp.p;
  }
  int rc = 0;
  const char* vb = "visual.transformer.resblocks.";
  const char* tb = "transformer.resblocks.";
  if (E->rn.on && nm.rfind("visual.", 0) == 0) {
    rc = rn_load(E, nm, p32, shape, ndim, s);
  } else if (nm.rfind(vb, 0) == 0 || nm.rfind(tb, 0) == 0) {
    const bool isv = nm.rfind(vb, 0) == 0;
    int layer; const char* tail;
    if (!parse_block_name(name + strlen(isv ? vb : tb), &layer, &tail)) return fail(E, MVLPT_ERR_ARG, "malformed block name: " + nm);
    rc = load_block_tensor(E, isv ? E->vis : E->txt, layer, tail, p32, shape, ndim, s);
  } else if (top) {
    if (!frozen_shape_ok(*top, shape, ndim)) return fail(E, MVLPT_ERR_ARG, "shape mismatch: " + nm);
    rc = frozen_load(E, *top, p32, shape, s);
  } else {
    return fail(E, MVLPT_ERR_ARG, "unknown frozen tensor name: " + nm);
  }
  if (rc) return rc;
  if (dtype != MVLPT_DT_F32) HIPCHK(E, hipStreamSynchronize(s));  // tmp is reused by the next call
  return 0;
}

int mvlpt_frozen_ready(void* h) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  const char* m = first_missing(E);
  if (m) return fail(E, MVLPT_ERR_STATE, std::string("frozen tensor not loaded: ") + m);
  return 0;
}

// ------------------------------------------------------------------------------------------------ image tower
// Blocks [from, to) of the image tower at full width, each behind its deep-prompt overwrite (or skipped, see below).  Returns 1 when
// it reaches the last block, which is CLS-only and run by mvlpt_image_fwd_resume.  R.ln1_ready is carried from block to block, and
// across the begin / resume cut.
static int image_blocks(Engine* E, int from, int to, hipStream_t s) {
  ImageRun& R = E->vrun; TowerState& st = R.st;
  const int B = R.B, n_vpt = R.n_vpt, n_deep = R.n_deep, dv = E->arch.vision_width, Lv = st.L;
  const float* const masks = R.mask;
  auto vmask = [&](int l) -> const float* { return masks ? masks + (size_t)l * B * n_vpt * dv : nullptr; };
  // ln_1 of block l can be folded when nothing touches the residual stream between FC2 of block l-1 and it: not behind a
  // deep-prompt overwrite, not behind a skipped block
  auto next_foldable = [&](int l) -> const LNp* {
    const int n = l + 1;
    if (!st.fold || n >= E->vis.layers) return nullptr;
    if (n_deep > 0) return nullptr;                       // rows 1..n_vpt are overwritten (or the block is skipped) in front of every later ln_1
    return &E->vis.blocks[n].ln1;
  };
  for (int l = from; l < to; ++l) {
    if (l > 0 && n_deep > 0) {
      if (l <= n_deep) {
        ProfScope ps(E, s, PC_GLUE, 0, (double)B * n_vpt * dv * 4.0);
        HIPCHK(E, launch_overwrite_rows(R.vpt_deep + (size_t)(l - 1) * n_vpt * dv, n_vpt, st.x[2 * l], B, Lv, dv, s, vmask(l)));
      } else {
        // reference quirk (trainers/mvlpt.py:71-83 has no `else`): the layer is skipped entirely
        st.skip[l] = 1;
        if (st.keep) {
          HIPCHK(E, hipMemcpyAsync(st.x[2 * l + 2], st.x[2 * l], (size_t)B * Lv * dv * 4, hipMemcpyDeviceToDevice, s));
        }
        continue;
      }
    }
    if (l == E->vis.layers - 1) return 1;      // the caller runs it on the CLS rows only
    if (R.packed) { if (int rc = block_fwd_packed(E, E->vis, st, l, s)) return rc; continue; }
    bool produced = false;
    if (int rc = block_fwd(E, E->vis, st, l, s, R.ln1_ready, next_foldable(l), &produced)) return rc;
    R.ln1_ready = produced;
  }
  return 0;
}

int mvlpt_image_fwd_begin(void* h, const void* image, int image_dtype, const float* vpt, const float* vpt_deep, int n_vpt, int n_deep,
                          int B, int save_for_bwd, int stop_block, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !image || B <= 0) return fail(E, MVLPT_ERR_ARG, "image_fwd: null/invalid argument");
  if (E->rn.on) return fail(E, MVLPT_ERR_UNSUPPORTED, std::string(kRefuseRN) + "image_fwd_begin");
  const bool wide = vision_wide(E);
  if (wide) {
    if (vpt || vpt_deep || n_vpt || n_deep) return fail(E, MVLPT_ERR_UNSUPPORTED, std::string(kRefuseWide) + "visual prompts");
    if (save_for_bwd) return fail(E, MVLPT_ERR_UNSUPPORTED, std::string(kRefuseWide) + "save_for_bwd");
    if (E->prec_mode == MVLPT_PREC_SPLIT_ALL)
      return fail(E, MVLPT_ERR_UNSUPPORTED, std::string(kRefuseWide) + "MVLPT_PREC_SPLIT_ALL (its forward-only towers run on pairs)");
  }
  ImageRun& R = E->vrun;
  if (R.phase == Phase::Pending) return fail(E, MVLPT_ERR_STATE, "image_fwd_begin: a forward is pending (call image_fwd_resume or image_fwd_abandon first)");
  if (int rc = mvlpt_frozen_ready(h)) return rc;
  if ((n_vpt > 0) != (vpt != nullptr)) return fail(E, MVLPT_ERR_ARG, "image_fwd: vpt pointer and n_vpt disagree");
  if ((n_deep > 0) != (vpt_deep != nullptr) || (n_deep > 0 && n_vpt <= 0)) return fail(E, MVLPT_ERR_ARG, "image_fwd: deep prompts need vpt");
  hipStream_t s = (hipStream_t)stream;
  const MvlptArch& A = E->arch;
  const int G = A.image_resolution / A.patch_size, G2 = G * G, dv = A.vision_width;
  const int Lv = 1 + n_vpt + G2;
  if (!wide && Lv > attn_max_len()) return fail(E, MVLPT_ERR_UNSUPPORTED, "image_fwd: sequence length > 256 not supported yet");
  const bool save = save_for_bwd != 0;
  const bool exact = E->prec_mode == MVLPT_PREC_SPLIT_ALL || (E->prec_mode == MVLPT_PREC_SPLIT_GRAD && save);
  const size_t X = exact ? 2 : 1;
  const size_t npatch = (size_t)B * G2;
  const bool gelu = E->act == ACT_GELU;
  R = ImageRun();      // opened: from here on the workspace no longer holds the last forward
  TowerState& st = R.st;
  void* patches; float* pe;
  if (int rc = carve_ws(E, E->vis_ws, "image_fwd_begin", kCarveSlack, [&](Bump& bp) {
        patches = bp.take_bytes(npatch * E->Kp * 2);
        pe = bp.take<float>(npatch * dv);
        carve_compact(bp, R.c, B, dv, X, gelu);
        TowerShape t;
        t.N = B; t.L = Lv; t.save = save; t.exact = exact; t.xs = split_kind(E); t.gelu = gelu;
        carve_tower(bp, E->vis, st, t);
      })) return rc;
  R.B = B; R.n_vpt = n_vpt; R.n_deep = n_deep; R.save = st.keep = save; R.vpt_deep = vpt_deep;
  st.fold = E->fold_mode >= 1 && (size_t)B * Lv >= (size_t)E->fold_min_rows && dv >= 256;
  if (st.fold) if (int rc = prepare_fold(E, s)) return rc;

  // the prompt dropout masks (mvlpt_set_vpt_dropout) belong to THIS forward and its backward only: taken over and cleared, then checked
  const Engine::VptMask m = std::exchange(E->vpt_mask, {});
  if (m.p && (n_vpt <= 0 || m.layers < 1 + n_deep || m.B != B || m.n != n_vpt))
    return fail(E, MVLPT_ERR_ARG, "image_fwd: the prompt dropout masks do not match this forward (layers >= 1 + n_deep, batch, n_vpt)");
  R.mask = m.p;
  { ProfScope ps(E, s, PC_GLUE, 0, (double)npatch * E->Kp * 6.0);
    HIPCHK(E, launch_patchify(E->dt, image, image_dtype, patches, B, A.image_resolution, A.patch_size, E->Kp, s)); }
  if (E->dbg_ck_on) { E->dbg_ck_n = 0; if (E->dbg_ck) (void)hipMemsetAsync(E->dbg_ck, 0, DBG_CK_MAX * sizeof(unsigned long long), s); }
  dbg_ck(E, patches, (size_t)npatch * E->Kp * 2, s);
  HIPCHK(E, gemm(E, EPI_STORE32, gemm_args(patches, (int)npatch, dv, E->Kp, pe), WRef{E->conv_w, 0, 0}, s));
  dbg_ck(E, pe, (size_t)npatch * dv * 4, s);
  // Packed residual stream (block_fwd_packed): fp16 tower, no prompts, nothing saved, every LayerNorm folded.  assemble_tokens
  // writes the rows in the packed format together with the row statistics of ln_1 of block 0.
  const int nt_d = dv / 128, ntp_d = (nt_d + 1) & ~1;
  const bool packed = E->resid_packed && E->dt == DT_F16 && !gelu && !save && !exact && st.fold && n_vpt == 0 && dv % 128 == 0 &&
                      ntp_d <= FOLD_NTP && E->vis.blocks[0].qkv.wg != nullptr;
  void* const xhi = st.x[0];
  uint8_t* const xlo = (uint8_t*)st.x[0] + (size_t)B * Lv * dv * 2;
  if (packed) {
    ProfScope ps(E, s, PC_GLUE, 0, (double)B * Lv * dv * 7.0);
    HIPCHK(E, launch_assemble_tokens_packed(pe, E->cls_emb, E->vpos, E->ln_pre.g, E->ln_pre.b, xhi, xlo, st.part[0], ntp_d, B, G2, dv, s));
    st.nt[0] = nt_d; st.ntp[0] = ntp_d;
    dbg_ck(E, xhi, (size_t)B * Lv * dv * 3, s); dbg_ck(E, st.part[0], (size_t)B * Lv * ntp_d * 8, s);
  } else {
    ProfScope ps(E, s, PC_GLUE, 0, (double)B * Lv * dv * 8.0);
    HIPCHK(E, launch_assemble_tokens(pe, E->cls_emb, E->vpos, E->ln_pre.g, E->ln_pre.b, vpt, n_vpt, st.x[0], B, G2, dv, s, R.mask));      // (layer 0's masks: the shallow prompts)
  }
  // blocks [0, stop_block); the last block (CLS rows only) always belongs to resume
  const int stop = std::min(std::max(stop_block, 0), E->vis.layers - 1);
  R.next = stop;
  R.packed = R.ln1_ready = packed;      // LayerNorm folding: the previous block's FC2 left this block's ln_1 input in folded form
  if (int rc = image_blocks(E, 0, stop, s)) return rc;
  R.phase = Phase::Pending;
  return 0;
}

int mvlpt_image_fwd_abandon(void* h) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  if (E->vrun.phase == Phase::Pending) E->vrun.phase = Phase::None;
  return 0;
}

int mvlpt_image_fwd_resume(void* h, float* feat_out, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !feat_out) return fail(E, MVLPT_ERR_ARG, "image_fwd_resume: null argument");
  if (E->rn.on) return fail(E, MVLPT_ERR_UNSUPPORTED, std::string(kRefuseRN) + "image_fwd_resume");
  ImageRun& R = E->vrun;
  if (R.phase != Phase::Pending) return fail(E, MVLPT_ERR_STATE, "image_fwd_resume: call image_fwd_begin first");
  R.phase = Phase::None;      // opened again: pending no longer, and nothing usable until the last statement
  hipStream_t s = (hipStream_t)stream;
  TowerState& st = R.st;
  const MvlptArch& A = E->arch;
  const int B = R.B, dv = A.vision_width, e = A.embed_dim, Lv = st.L;
  const int rest = image_blocks(E, R.next, E->vis.layers, s);
  if (rest < 0) return rest;
  R.last_compact = rest == 1;
  if (rest == 1) {      // the last block, CLS rows only (mvlpt_image_bwd: only the CLS query carries a gradient into its attention)
    if (int rc = last_block_fwd(E, E->vis, st, R.c, LastRows{nullptr, 1, E->ln_post}, R.packed, R.ln1_ready, s)) return rc;
  } else {
    // ln_post on the CLS row, then @ proj   (trainers/mvlpt.py:88-91)
    LnFwdArgs ln = ln_args(st.x[2 * E->vis.layers], E->ln_post, R.c.out32, B, dv);
    ln.row_mul = Lv;
    HIPCHK(E, ln_fwd(E, DT_F32, ln, s));
  }
  { ProfScope ps(E, s, PC_HEAD, 2.0 * B * e * dv, 4.0 * ((double)B * dv + (double)e * dv + (double)B * e));
    HIPCHK(E, launch_sgemm_bt(R.c.out32, E->vproj_t, feat_out, B, e, dv, nullptr, s)); }
  R.phase = R.save ? Phase::Saved : Phase::Done;
  return 0;
}

int mvlpt_image_fwd(void* h, const void* image, int image_dtype, const float* vpt, const float* vpt_deep, int n_vpt, int n_deep,
                    int B, float* feat_out, int save_for_bwd, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !image || !feat_out || B <= 0) return fail(E, MVLPT_ERR_ARG, "image_fwd: null/invalid argument");
  if (E->rn.on) {
    if (vpt || vpt_deep || n_vpt || n_deep) return fail(E, MVLPT_ERR_UNSUPPORTED, std::string(kRefuseRN) + "visual prompts");
    if (save_for_bwd) return fail(E, MVLPT_ERR_UNSUPPORTED, std::string(kRefuseRN) + "save_for_bwd");
    if (int rc = mvlpt_frozen_ready(h)) return rc;
    return resnet_fwd(E, image, image_dtype, B, feat_out, (hipStream_t)stream);
  }
  if (int rc = mvlpt_image_fwd_begin(h, image, image_dtype, vpt, vpt_deep, n_vpt, n_deep, B, save_for_bwd, E->vis.layers, stream)) return rc;
  return mvlpt_image_fwd_resume(h, feat_out, stream);
}

int mvlpt_image_bwd(void* h, const float* dfeat, float* dvpt, float* dvpt_deep, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !dfeat) return fail(E, MVLPT_ERR_ARG, "image_bwd: null argument");
  if (E->rn.on) return fail(E, MVLPT_ERR_UNSUPPORTED, std::string(kRefuseRN) + "image_bwd");
  if (vision_wide(E)) return fail(E, MVLPT_ERR_UNSUPPORTED, std::string(kRefuseWide) + "image_bwd");
  ImageRun& R = E->vrun; TowerState& st = R.st;
  if (R.phase == Phase::Pending) return fail(E, MVLPT_ERR_STATE, "image_bwd: a forward is pending between image_fwd_begin and image_fwd_resume");
  if (!bwd_ready(R.phase)) return fail(E, MVLPT_ERR_STATE, "image_bwd: call image_fwd(save_for_bwd=1) first");
  if ((R.n_vpt > 0 && !dvpt) || (R.n_deep > 0 && !dvpt_deep)) return fail(E, MVLPT_ERR_ARG, "image_bwd: missing gradient output");
  hipStream_t s = (hipStream_t)stream;
  const MvlptArch& A = E->arch;
  const int B = R.B, dv = A.vision_width, e = A.embed_dim, Lv = st.L, n = R.n_vpt;
  const size_t T = (size_t)B * Lv;
  { ProfScope ps(E, s, PC_GLUE, 0, (double)T * dv * 10.0);
    HIPCHK(E, launch_grad_scale(dfeat, (size_t)B * e, 64.0f, st.scale_dev, s));
    HIPCHK(E, launch_sgemm_bt(dfeat, E->vproj, R.c.dout32, B, dv, e, st.scale_dev, s)); }
  { ProfScope ps(E, s, PC_GLUE, 0, (double)T * dv * 4.0);
    HIPCHK(E, launch_zero(st.dx32, T * dv * 4, s)); }
  int l_top = st.layers - 1;
  const int xs = st.xs;
  // gradient of the deep prompts of block l (its input rows 1..n), which then stop carrying one
  auto reduce_deep = [&](int l) -> int {
    if (!(l > 0 && R.n_deep > 0 && l <= R.n_deep)) return 0;
    ProfScope ps(E, s, PC_GLUE, 0, (double)B * n * dv * 10.0);
    HIPCHK(E, launch_reduce_prompt_rows(E->dt, st.dx32, st.dx16, B, Lv, dv, 1, n, dvpt_deep + (size_t)(l - 1) * n * dv,
                                        st.scale_dev, 1, s, xs, R.mask ? R.mask + (size_t)l * B * n * dv : nullptr));
    return 0;
  };
  if (R.last_compact) {      // last block, CLS rows only (see mvlpt_image_fwd_resume)
    if (int rc = last_block_bwd(E, E->vis, st, R.c, LastRows{nullptr, 1, E->ln_post}, s)) return rc;
    if (int rc = reduce_deep(l_top)) return rc;
    --l_top;
  } else {
    LnBwdArgs ln = ln_bwd_args(R.c.dout32, st.x[2 * st.layers], E->ln_post, st.dx32, B, dv);
    ln.row_mul = Lv;
    HIPCHK(E, ln_bwd(E, ln, s));
    { ProfScope ps(E, s, PC_GLUE, 0, (double)T * dv * 6.0);
      if (xs) HIPCHK(E, launch_cast_f32_split(E->dt, st.dx32, st.dx16, T, dv, nullptr, s, xs == 2));
      else HIPCHK(E, launch_cast_f32_to16(E->dt, st.dx32, st.dx16, T * dv, nullptr, s)); }
  }
  for (int l = l_top; l >= 0; --l) {
    if (st.skip[l]) continue;
    if (int rc = block_bwd(E, E->vis, st, l, s)) return rc;
    if (int rc = reduce_deep(l)) return rc;
  }
  if (n > 0) {
    ProfScope ps(E, s, PC_GLUE, 0, (double)B * n * dv * 4.0);
    HIPCHK(E, launch_reduce_prompt_rows(E->dt, st.dx32, st.dx16, B, Lv, dv, 1, n, dvpt, st.scale_dev, 0, s, 0, R.mask));
  }
  R.phase = Phase::BwdDone;
  return 0;
}

// ------------------------------------------------------------------------------------------------ class ranges
// Host side of the ranged tower / head: class_lo / class_hi [G] (host arrays) -> t = [lo (G) | start (G + 1) | seq_cls (S) | seq_grp (S)],
// checked here so that no kernel can index outside the class tables.  Returns S (the number of sequences), or -1 for a bad range.
static int64_t build_range_table(const int32_t* class_lo, const int32_t* class_hi, int G, int C, std::vector<int32_t>& t) {
  int64_t S = 0;
  for (int g = 0; g < G; ++g) {
    if (class_lo[g] < 0 || class_lo[g] > class_hi[g] || class_hi[g] > C) return -1;
    S += class_hi[g] - class_lo[g];
  }
  if (S > INT32_MAX) return -1;
  t.resize((size_t)2 * G + 1 + 2 * (size_t)S);
  int32_t *lo = t.data(), *start = lo + G, *cls = start + G + 1, *grp = cls + S;
  int32_t s = 0;
  for (int g = 0; g < G; ++g) {
    lo[g] = class_lo[g]; start[g] = s;
    for (int c = class_lo[g]; c < class_hi[g]; ++c, ++s) { cls[s] = c; grp[s] = g; }
  }
  start[G] = s;
  return S;
}

// ------------------------------------------------------------------------------------------------ text tower
static_assert(sizeof(MvlptTextJob) == MVLPT_TEXT_JOB_BYTES, "MvlptTextJob has no implicit padding");
// One text forward: the caller's job (its fields: include/mvlpt_hip.h) and what text_job_check derives from it.
// Plain (and deep, n_deep > 0): C = Cg = n_cls sequences, G = 0.  Ranged: G = groups over the [Cg = n_cls, ...] class tables, C = S
// sequences described by E->t_range_host.  Ids: mvlpt_text_encode_tokens, C sequences of token ids (E->t_ids_host); no class tables
// and no ctx.
struct TextJob : MvlptTextJob {
  TextKind kind = TextKind::Plain;
  int C = 0, Cg = 0, G = 0;
  explicit TextJob(const MvlptTextJob& job = MvlptTextJob{}) : MvlptTextJob(job) {}
};
// What a text forward over C sequences of length L carves from txt_ws: text_fwd_impl carves with it and mvlpt_text_workspace_bytes
// counts with it.  `exact`: split operands (see mvlpt_text_fwd); ctx_rows: rows of the ctx_pos table; range_ints / ids_ints: the range
// table of a ranged forward and the id table of mvlpt_text_encode_tokens (0: none, a null pointer).  A saving tower is carved under the
// engine's activation-checkpointing setting (mvlpt_set_text_act_ckpt).
// Lg: the gradient length of a saving tower (text_grad_len below; L: every position).  P: the shared prefix (text_prefix_len).
struct TextShape {
  int C = 0, L = 0;
  bool save = false, exact = false;
  size_t ctx_rows = 0, range_ints = 0, ids_ints = 0;
  int Lg = 0, P = 0;
};
static void text_layout(Bump& bp, const Engine* E, TextRun& R, const TextShape& t) {
  const bool gelu = E->act == ACT_GELU;
  carve_compact(bp, R.c, t.C, E->arch.text_width, t.exact ? 2 : 1, gelu);
  R.eot_rows = bp.take<int32_t>(t.C);
  R.ctx_pos = bp.take<int32_t>(t.ctx_rows);
  R.range = t.range_ints ? bp.take<int32_t>(t.range_ints) : nullptr;
  R.ids = t.ids_ints ? bp.take<int32_t>(t.ids_ints) : nullptr;
  TowerShape w;
  w.N = t.C; w.L = t.L; w.Lg = t.Lg; w.P = t.P;
  w.save = t.save; w.causal = true; w.exact = t.exact; w.xs = split_kind(E); w.gelu = gelu; w.segments = E->text_act_ckpt;
  if (t.P > 0) { w.N = t.C + 1; w.L = t.L - t.P; w.Lg = t.Lg - t.P; }      // (a shared prefix: C + 1 slots of L - P rows, TowerState::P)
  carve_tower(bp, E->txt, R.st, w);
}
// The shared prefix a plain forward runs under (mvlpt_set_text_shared_prefix): the setting, lowered until the prefix fits a gradient
// slot (P <= Lg - P) and a slot keeps MVLPT_TEXT_MIN_L rows (Lg - P >= 3); 0 on every route that does not take one: class-specific or
// deep contexts, the ranged and token-id towers, activation checkpointing, sequences the short kernels do not take.  Split and single
// operands alike (attention32.hip / attention.hip).  `setting`: what the forward took out of Engine::text_shared_prefix.
static int text_prefix_len(const Engine* E, int setting, const TextJob& j, int Lg) {
  if (setting <= 0 || j.kind != TextKind::Plain || j.ctx_per_class || j.n_ctx <= 0 || j.n_deep > 0 || j.L > 80 || E->text_act_ckpt != 1)
    return 0;
  int P = std::min(setting, j.L - 1);
  P = std::min(P, std::min(Lg / 2, Lg - 3));
  return P > 0 ? P : 0;
}
// The gradient length a saving forward over sequences of L positions runs under (mvlpt_set_text_grad_len): the setting, at most L
static int text_grad_len(const Engine* E, int L) { return E->text_grad_len > 0 && E->text_grad_len < L ? E->text_grad_len : L; }
// The published figure is the count plus 8192 bytes: the Python chunk planners compare it with budgets, so it stays where it is, to the byte.
constexpr size_t kTextSlack = 2 * kCarveSlack;
// mvlpt_text_workspace_bytes publishes the count with ctx_rows = C * (L - 2), the largest n_ctx a forward accepts, and no tables.  A ranged
// forward over S sequences in G <= S groups of a class table no longer than S also reserves its range table, 2 G + 1 + 2 S
// <= 4 S + 1 ints, and uses S * n_ctx of the ctx_pos rows, so the published figure still bounds the reservation whenever
// S * (L - 2 - n_ctx) >= 4 S + 1 + 128 ints (the 128 cover the two roundings to 256 bytes): n_ctx <= L - 7 from S = 129 sequences on,
// n_ctx <= L - 8 from S = 65, the trainers' n_ctx = 4 or 16 at L = 77 from S = 3.  It does not when n_ctx is close to L - 2 (or for
// a ranged forward over fewer sequences than classes); the reservation then exceeds it by at most 16 S + 514 bytes, and txt_ws
// grows on demand.
static bool text_exact(const Engine* E) { return E->prec_mode == MVLPT_PREC_SPLIT_ALL || E->prec_mode == MVLPT_PREC_SPLIT_GRAD; }

// Full-width text blocks first .. end-1 of one checkpoint segment (a tower without checkpointing is one `last` segment), starting
// from the stand-alone ln_1.  Only the last segment hands a folded ln_1 on to the block behind it (the compact last block); a
// checkpointed one closes with the plain residual epilogue, so that the segment behind it starts the same way in the first pass and
// in the backward's recomputation.  *ln1_ready: what the block behind `end - 1` finds.
// Deep text prompts: the context rows of block l's input (1 <= l <= n_deep) are replaced by ctx_deep[l - 1] in front of the block, in
// the first pass and in the recomputation alike (writing a segment's boundary buffer twice writes the same values).
static int text_deep_overwrite(Engine* E, int l, hipStream_t s) {
  const TextRun& R = E->trun; const TowerState& st = R.st;
  if (l < 1 || l > R.n_deep) return 0;
  const int dtw = st.d, n = R.n_ctx;
  ProfScope ps(E, s, PC_GLUE, 0, (double)st.N * n * dtw * 4.0);
  HIPCHK(E, launch_overwrite_ctx_rows(R.ctx_deep + (size_t)(l - 1) * n * dtw, R.ctx_pos, st.x[2 * l], st.N, st.L, dtw, n, s));
  return 0;
}
// keep: this pass writes what a backward reads (false: the first pass of a checkpointed segment)
static int text_segment_fwd(Engine* E, int first, int end, bool last, bool keep, bool* ln1_ready, hipStream_t s) {
  TowerState& st = E->trun.st;
  st.keep = keep; *ln1_ready = false;
  for (int l = first; l < end; ++l) {
    if (int rc = text_deep_overwrite(E, l, s)) return rc;
    bool produced = false;
    // (ln_1 of a block behind an overwrite is not folded: its input rows change after the FC2 in front of it wrote them)
    const bool next = st.fold && (last || l + 1 < end) && l + 1 > E->trun.n_deep;
    if (int rc = block_fwd(E, E->txt, st, l, s, *ln1_ready, next ? &E->txt.blocks[l + 1].ln1 : nullptr, &produced)) return rc;
    *ln1_ready = produced;
  }
  return 0;
}

// The text tower over the j.C sequences of one TextJob
static int text_fwd_impl(Engine* E, const TextJob& j, float* feat_out, mvlpt_stream_t stream) {
  const bool ranged = j.kind == TextKind::Ranged, ids = j.kind == TextKind::Ids;
  const int C = j.C, L = j.L, n_ctx = j.n_ctx, n_deep = j.n_deep, G = j.G, Cg = j.Cg;
  // one-shot, taken before any check can refuse the call: the caller's proof holds for the tables of THIS forward only, whichever
  // entry it came through and whether or not it runs
  const int prefix_setting = E->text_shared_prefix;
  E->text_shared_prefix = 0;
  if (int rc = mvlpt_frozen_ready(E)) return rc;
  if ((n_ctx > 0) != (j.ctx != nullptr) || n_ctx < 0 || n_ctx > L - 2) return fail(E, MVLPT_ERR_ARG, "text_fwd: ctx pointer and n_ctx disagree");
  const MvlptArch& A = E->arch;
  if (L > A.context_length) return fail(E, MVLPT_ERR_ARG, "text_fwd: L exceeds context_length");
  if (L > attn_max_len()) return fail(E, MVLPT_ERR_UNSUPPORTED, "text_fwd: L > 256");
  hipStream_t s = (hipStream_t)stream;
  const int dtw = A.text_width, e = A.embed_dim;
  const bool save = j.save_for_bwd != 0;
  // The text tower runs with split operands in every mode but MVLPT_PREC_FAST, also when nothing is saved for a backward:
  // n_ctx == 0: the features are constants of the run (computed once and cached by the caller) that enter every
  // image-side gradient through the logits; inference (model_inference, trainers/mvlpt.py:986-987): they are computed once
  // per parameter version, not per batch, so the extra matrix time does not recur — and single operands leave 5-9e-4 on the text
  // features, which put the inference logits of 5 of the 18 reference fixtures outside 1e-3 (profiles/r04_inference_parity.txt)
  const bool exact = text_exact(E);
  // ctx_pos is per class for the ranged tower, which may run fewer sequences than there are classes
  TextShape shape;
  shape.C = C; shape.L = L; shape.save = save; shape.exact = exact;
  shape.ctx_rows = (size_t)(ranged && Cg > C ? Cg : C) * (n_ctx > 0 ? n_ctx : 1);
  const size_t range_ints = shape.range_ints = ranged ? E->t_range_host.size() : 0;
  const size_t ids_ints = shape.ids_ints = ids ? E->t_ids_host.size() : 0;
  // a gradient that stops in front of an EOT row would be wrong (never out of bounds): refused before anything is launched
  const int Lg = shape.Lg = save ? text_grad_len(E, L) : L;
  if (Lg < L && Lg <= E->text_max_eot)
    return fail(E, MVLPT_ERR_ARG, "text_fwd: the gradient length (mvlpt_set_text_grad_len) does not reach the largest EOT position");
  const int P = shape.P = text_prefix_len(E, prefix_setting, j, Lg);
  TextRun& R = E->trun = TextRun();      // opened: from here on the workspace no longer holds the last forward
  TowerState& st = R.st;
  if (int rc = carve_ws(E, E->txt_ws, "text_fwd", kTextSlack, [&](Bump& bp) { text_layout(bp, E, R, shape); })) return rc;
  if (P > 0) {      // the sum over more than 512 classes enters slot 0 scaled down by a power of two (TowerState::part_mul)
    int sh = 0;
    while (((int64_t)512 << sh) < C) ++sh;
    st.part_mul = std::ldexp(1.0f, -sh);
  }
  R.C = C; R.L = L; R.n_ctx = n_ctx; R.per_class = j.ctx_per_class; R.kind = j.kind; R.groups = G;
  R.n_deep = n_deep; R.ctx_deep = n_deep > 0 ? j.ctx_deep : nullptr;
  st.fold = E->fold_mode >= 2 && (size_t)C * L >= (size_t)E->fold_min_rows && dtw >= 256;
  if (st.fold) if (int rc = prepare_fold(E, s)) return rc;
  if (ids) {
    ProfScope ps(E, s, PC_GLUE, 0, (double)C * L * dtw * 12.0);
    HIPCHK(E, hipMemcpyAsync(R.ids, E->t_ids_host.data(), ids_ints * 4, hipMemcpyHostToDevice, s));
    HIPCHK(E, hipMemcpyAsync(R.eot_rows, R.ids + (size_t)C * L, (size_t)C * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(E, launch_embed_tokens(E->tok_emb, E->tpos, R.ids, L, st.x[0], C, L, dtw, s));
  } else
  { ProfScope ps(E, s, PC_GLUE, 0, (double)C * L * dtw * 12.0);
    if (ranged) {
      const int32_t *seq_cls = R.range + 2 * G + 1, *seq_grp = seq_cls + C;
      HIPCHK(E, hipMemcpyAsync(R.range, E->t_range_host.data(), range_ints * 4, hipMemcpyHostToDevice, s));
      HIPCHK(E, launch_assemble_prompts_ranged(j.prefix, j.suffix, j.ctx, n_ctx, j.layout, E->tpos, st.x[0], seq_cls, seq_grp, C, L, dtw, s));
      HIPCHK(E, launch_eot_rows_ranged(j.eot, R.eot_rows, seq_cls, C, L, s));
      if (save) HIPCHK(E, launch_build_ctx_pos(j.layout, R.ctx_pos, Cg, L, n_ctx, s));     // per class: [Cg, n_ctx]
    } else {
      HIPCHK(E, launch_assemble_prompts(j.prefix, j.suffix, j.ctx, j.ctx_per_class, n_ctx, j.layout, E->tpos, st.x[0], C, L, dtw, s, P));
      HIPCHK(E, launch_eot_rows(j.eot, R.eot_rows, C, L, s, P));
      if ((save || n_deep > 0) && n_ctx > 0) HIPCHK(E, launch_build_ctx_pos(j.layout, R.ctx_pos, C, L, n_ctx, s, P, st.Lg));
    } }
  // Checkpointed segments (every one but the last, st.seg) run as a tower that saves nothing; their closing block writes the next
  // segment's boundary buffer.  No ln_1 is folded across a segment boundary, so mvlpt_text_bwd can repeat a segment launch for launch.
  bool ln1_ready = false;
  const int k = (int)st.seg.size() - 1;
  for (int i = 0; i < k; ++i)
    if (int rc = text_segment_fwd(E, st.seg[i], std::min(st.seg[i + 1], E->txt.layers - 1), i == k - 1, save && i == k - 1, &ln1_ready, s))
      return rc;
  // the last block on the C gathered EOT rows
  st.keep = save;
  if (int rc = text_deep_overwrite(E, E->txt.layers - 1, s)) return rc;
  if (int rc = last_block_fwd(E, E->txt, st, R.c, LastRows{R.eot_rows, 0, E->ln_final}, false, ln1_ready, s)) return rc;
  { ProfScope ps(E, s, PC_HEAD, 2.0 * C * e * dtw, 4.0 * ((double)C * dtw + (double)e * dtw + (double)C * e));
    HIPCHK(E, launch_sgemm_bt(R.c.out32, E->tproj_t, feat_out, C, e, dtw, nullptr, s)); }
  R.phase = save ? Phase::Saved : Phase::Done;
  return 0;
}

// Every refusal of a job for what it says (text_fwd_impl adds those that depend on the engine's settings), and the derived fields.
// Nothing is launched and, up to the range table (host scratch no saved forward reads), no engine state is touched.
static int text_job_check(Engine* E, TextJob& j, const float* feat_out) {
  if (!j.prefix || !j.suffix || !j.layout || !j.eot || !feat_out || j.n_cls <= 0 || j.L <= 0 || j.reserved != 0)
    return fail(E, MVLPT_ERR_ARG, "text_fwd: null/invalid argument");
  const bool ranged = j.class_lo || j.class_hi;
  if (!j.class_lo != !j.class_hi || ranged != (j.groups != 0))
    return fail(E, MVLPT_ERR_ARG, "text_fwd: class_lo, class_hi and groups come together");
  if (j.n_deep < 0) return fail(E, MVLPT_ERR_ARG, "text_fwd: n_deep is negative");
  if (j.n_deep > 0) {
    if (ranged) return fail(E, MVLPT_ERR_ARG, "text_fwd: deep prompts are not offered on the ranged tower");
    if (j.ctx_per_class) return fail(E, MVLPT_ERR_ARG, "text_fwd: deep prompts take a generic context (ctx_per_class = 0)");
    if (!j.ctx_deep) return fail(E, MVLPT_ERR_ARG, "text_fwd: ctx_deep is null with n_deep > 0");
    if (j.n_ctx <= 0) return fail(E, MVLPT_ERR_ARG, "text_fwd: deep prompts need context tokens (n_ctx == 0)");
    if (j.n_deep > E->txt.layers - 1)
      return fail(E, MVLPT_ERR_ARG, "text_fwd: n_deep exceeds text_layers - 1 (block 0 reads the embedding-level context)");
  }
  j.C = j.Cg = j.n_cls;
  if (!ranged) return 0;
  if (!j.ctx || j.ctx_per_class || j.groups < 0 || j.n_ctx <= 0) return fail(E, MVLPT_ERR_ARG, "text_fwd: null/invalid argument");
  if (j.groups > 65535) return fail(E, MVLPT_ERR_ARG, "text_fwd: too many groups");
  const int64_t S = build_range_table(j.class_lo, j.class_hi, j.groups, j.n_cls, E->t_range_host);
  if (S < 0) return fail(E, MVLPT_ERR_ARG, "text_fwd: a class range is not inside [0, C] or the ranges hold too many sequences");
  if (S == 0) return fail(E, MVLPT_ERR_ARG, "text_fwd: every range is empty");
  if (S > (int64_t)INT32_MAX / j.L) return fail(E, MVLPT_ERR_ARG, "text_fwd: too many sequences");
  j.kind = TextKind::Ranged; j.G = j.groups; j.C = (int)S;
  return 0;
}

int mvlpt_text_fwd(void* h, const MvlptTextJob* job, float* feat_out, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !job) return fail(E, MVLPT_ERR_ARG, "text_fwd: null/invalid argument");
  TextJob j(*job);
  if (int rc = text_job_check(E, j, feat_out)) return rc;
  return text_fwd_impl(E, j, feat_out, stream);
}

// CLIP.encode_text (clip/model.py:343-356) over S sequences of token ids, trimmed to their first L positions
int mvlpt_text_encode_tokens(void* h, const int32_t* ids, int ld, int S, int L, float* feat_out, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !ids || !feat_out || S <= 0 || L <= 0 || ld < L) return fail(E, MVLPT_ERR_ARG, "text_encode_tokens: null/invalid argument");
  if (!E->tok_emb || E->vocab <= 0)
    return fail(E, MVLPT_ERR_STATE, "text_encode_tokens: token_embedding.weight is not loaded (mvlpt_load_frozen)");
  if (L < MVLPT_TEXT_MIN_L) return fail(E, MVLPT_ERR_ARG, "text_encode_tokens: L is below MVLPT_TEXT_MIN_L");
  if (L > E->arch.context_length) return fail(E, MVLPT_ERR_ARG, "text_encode_tokens: L exceeds context_length");
  if (S > 65535) return fail(E, MVLPT_ERR_ARG, "text_encode_tokens: more than 65535 sequences (the attention launches put the sequence on grid.y)");
  // every id the kernel will read is checked here, and the EOT row (first occurrence of the row maximum over all ld columns, as
  // text.argmax(dim=-1)) must lie inside the trimmed sequence; nothing is launched for a bad table
  std::vector<int32_t>& t = E->t_ids_host;
  t.resize((size_t)S * L + S);
  int32_t* rows = t.data() + (size_t)S * L;
  for (int q = 0; q < S; ++q) {
    const int32_t* r = ids + (size_t)q * ld;
    int arg = 0;
    for (int i = 1; i < ld; ++i) if (r[i] > r[arg]) arg = i;
    if (arg >= L) return fail(E, MVLPT_ERR_ARG, "text_encode_tokens: the EOT position of sequence " + std::to_string(q) + " is not below L");
    for (int i = 0; i < L; ++i) {
      if (r[i] < 0 || r[i] >= E->vocab)
        return fail(E, MVLPT_ERR_ARG, "text_encode_tokens: token id outside [0, vocab) in sequence " + std::to_string(q));
      t[(size_t)q * L + i] = r[i];
    }
    rows[q] = q * L + arg;
  }
  TextJob j;
  j.kind = TextKind::Ids;
  j.Cg = j.C = S; j.L = L;
  return text_fwd_impl(E, j, feat_out, stream);
}

int mvlpt_text_ensemble(const float* feats, int T, int C, int e, float* out, mvlpt_stream_t stream) {
  if (!feats || !out || T <= 0 || C <= 0 || e <= 0) return fail(nullptr, MVLPT_ERR_ARG, "text_ensemble: null/invalid argument");
  const hipError_t rc = launch_ensemble_features(feats, out, T, C, e, (hipStream_t)stream);
  if (rc != hipSuccess) return fail(nullptr, MVLPT_ERR_HIP, std::string("text_ensemble: ") + hipGetErrorString(rc));
  return 0;
}

int mvlpt_set_text_act_ckpt(void* h, int segments) {
  Engine* E = (Engine*)h;
  if (!E) return fail(E, MVLPT_ERR_ARG, "set_text_act_ckpt: null handle");
  if (segments < 1) return fail(E, MVLPT_ERR_ARG, "set_text_act_ckpt: segments must be at least 1");
  E->text_act_ckpt = segments;      // clamped to the layer count where it is used (ckpt_plan)
  return 0;
}

int mvlpt_set_text_grad_len(void* h, int grad_len, int max_eot) {
  Engine* E = (Engine*)h;
  if (!E) return fail(E, MVLPT_ERR_ARG, "set_text_grad_len: null handle");
  if (grad_len < MVLPT_TEXT_MIN_L || grad_len > E->arch.context_length)
    return fail(E, MVLPT_ERR_ARG, "set_text_grad_len: the gradient length must lie in [MVLPT_TEXT_MIN_L, context_length]");
  if (max_eot < 0) return fail(E, MVLPT_ERR_ARG, "set_text_grad_len: max_eot is negative");
  E->text_grad_len = grad_len; E->text_max_eot = max_eot;      // read by the next saving text forward, which records what it ran under
  return 0;
}

int mvlpt_set_text_shared_prefix(void* h, int prefix) {
  Engine* E = (Engine*)h;
  if (!E) return fail(E, MVLPT_ERR_ARG, "set_text_shared_prefix: null handle");
  if (prefix < 0 || prefix >= E->arch.context_length)
    return fail(E, MVLPT_ERR_ARG, "set_text_shared_prefix: the prefix must lie in [0, context_length)");
  E->text_shared_prefix = prefix;      // consumed by the next text forward, which records what it ran under (TowerState::P)
  return 0;
}

int mvlpt_text_act_ckpt_plan(void* h, int32_t* first_layer, int cap, int* n_segments) {
  Engine* E = (Engine*)h;
  if (!E || !first_layer || !n_segments || cap < 0) return fail(E, MVLPT_ERR_ARG, "text_act_ckpt_plan: null/invalid argument");
  const std::vector<int> seg = ckpt_plan(E->txt.layers, E->text_act_ckpt);
  const int k = (int)seg.size() - 1;
  *n_segments = k;
  if (cap < k) return fail(E, MVLPT_ERR_ARG, "text_act_ckpt_plan: first_layer holds fewer than n_segments entries");
  for (int i = 0; i < k; ++i) first_layer[i] = seg[i];
  return 0;
}

int mvlpt_text_workspace_bytes(void* h, int C_total, int L, int save_for_bwd, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E || !out || C_total <= 0 || L <= 2) return fail(E, MVLPT_ERR_ARG, "text_workspace_bytes: null/invalid argument");
  // the ctx_pos table is sized for the largest n_ctx a forward accepts (L - 2): at most C_total * L * 4 bytes over the exact figure
  // a counting pass into scratch state: a saved forward whose backward has not run keeps its own
  TextRun scratch;
  TextShape shape;
  shape.C = C_total; shape.L = shape.Lg = L; shape.save = save_for_bwd != 0; shape.exact = text_exact(E);
  shape.ctx_rows = (size_t)C_total * (L - 2);
  *out = (int64_t)(carve_count([&](Bump& bp) { text_layout(bp, E, scratch, shape); }) + kTextSlack);
  return 0;
}

// The backward of every text forward.  dctx_deep: the gradient of the deep prompts, there exactly when the forward ran some.
int mvlpt_text_bwd(void* h, const float* dfeat, float* dctx, float* dctx_deep, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !dfeat || !dctx) return fail(E, MVLPT_ERR_ARG, "text_bwd: null argument");
  TextRun& R = E->trun; TowerState& st = R.st;
  if (R.phase == Phase::Consumed)
    return fail(E, MVLPT_ERR_STATE, "text_bwd: a backward under activation checkpointing has consumed the saved state; run the forward again");
  if (!bwd_ready(R.phase)) return fail(E, MVLPT_ERR_STATE, "text_bwd: call text_fwd(save_for_bwd=1) first");
  if (R.n_ctx <= 0) return fail(E, MVLPT_ERR_STATE, "text_bwd: the forward had no context tokens");
  if (R.n_deep > 0 && !dctx_deep) return fail(E, MVLPT_ERR_ARG, "text_bwd: dctx_deep is null after a forward with deep prompts");
  if (R.n_deep == 0 && dctx_deep) return fail(E, MVLPT_ERR_ARG, "text_bwd: dctx_deep is set after a forward without deep prompts");
  hipStream_t s = (hipStream_t)stream;
  const MvlptArch& A = E->arch;
  // L: the gradient length this forward was saved under (TowerState::Lg), the sequence pitch of every gradient buffer
  // (under a shared prefix the buffers hold C + 1 slots of L rows: TowerState::P)
  const int C = R.C, L = st.Lg, dtw = A.text_width, e = A.embed_dim;
  const size_t T = (size_t)st.N * L;
  { ProfScope ps(E, s, PC_GLUE, 0, (double)T * dtw * 10.0);
    HIPCHK(E, launch_grad_scale(dfeat, (size_t)C * e, 64.0f, st.scale_dev, s));
    HIPCHK(E, launch_sgemm_bt(dfeat, E->tproj, R.c.dout32, C, dtw, e, st.scale_dev, s)); }
  { ProfScope ps(E, s, PC_GLUE, 0, (double)T * dtw * 4.0);
    HIPCHK(E, launch_zero(st.dx32, T * dtw * 4, s)); }
  // the plan of the forward that saved this state (st.seg), not the engine's current setting
  const int k = (int)st.seg.size() - 1;
  if (k > 1) R.phase = Phase::Consumed;      // from here on the slots no longer hold what the forward left
  // gradient of the deep prompts of block l (its input's context rows), which then stop carrying one into block l - 1
  auto gather_deep = [&](int l) -> int {
    if (l < 1 || l > R.n_deep) return 0;
    const int n = R.n_ctx;
    ProfScope ps(E, s, PC_GLUE, 0, (double)C * n * dtw * 10.0);
    HIPCHK(E, launch_gather_zero_ctx_grad(E->dt, st.dx32, st.dx16, st.xs, R.ctx_pos, C, L, dtw, n, dctx_deep + (size_t)(l - 1) * n * dtw,
                                          st.scale_dev, s));
    return 0;
  };
  if (int rc = last_block_bwd(E, E->txt, st, R.c, LastRows{R.eot_rows, 0, E->ln_final}, s)) return rc;      // the last block on the C compact EOT rows
  if (int rc = gather_deep(st.layers - 1)) return rc;
  for (int l = st.layers - 2; l >= st.seg[k - 1]; --l) {
    if (int rc = block_bwd(E, E->txt, st, l, s)) return rc;
    if (int rc = gather_deep(l)) return rc;
  }
  // checkpointed segments, from the back: the forward's launches again from the segment's input, this time keeping lse / u, into
  // the slots the segment behind it no longer needs; then its backward
  for (int i = k - 2; i >= 0; --i) {
    bool ln1_ready = false;
    if (int rc = text_segment_fwd(E, st.seg[i], st.seg[i + 1], false, true, &ln1_ready, s)) return rc;
    for (int l = st.seg[i + 1] - 1; l >= st.seg[i]; --l) {
      if (int rc = block_bwd(E, E->txt, st, l, s)) return rc;
      if (int rc = gather_deep(l)) return rc;
    }
  }
  { ProfScope ps(E, s, PC_GLUE, 0, (double)C * R.n_ctx * dtw * 4.0);
    if (R.kind == TextKind::Ranged)
      HIPCHK(E, launch_gather_ctx_grad_ranged(st.dx32, R.ctx_pos, R.range, R.range + R.groups, R.groups, L, dtw, R.n_ctx, dctx, st.scale_dev, s));
    else
      HIPCHK(E, launch_gather_ctx_grad(st.dx32, R.ctx_pos, C, L, dtw, R.n_ctx, R.per_class, dctx, st.scale_dev, s, st.P, 1.f / st.part_mul)); }
  if (k == 1) R.phase = Phase::BwdDone;
  return 0;
}

// ------------------------------------------------------------------------------------------------ head
// The normalised rows and norms of B image and C text features; the ranged head's table of `ints` ints behind them (*tab)
static int head_carve(Engine* E, const char* who, int B, int C, size_t ints = 0, int32_t** tab = nullptr) {
  const int e = E->arch.embed_dim;
  HeadRun& R = E->hrun;
  return carve_ws(E, E->head_ws, who, kCarveSlack, [&](Bump& bp) {
    R.imn = bp.take<float>((size_t)B * e); R.txn = bp.take<float>((size_t)C * e);
    R.inorm = bp.take<float>(B); R.tnorm = bp.take<float>(C);
    if (tab) *tab = bp.take<int32_t>(ints);
  });
}

int mvlpt_logits_fwd(void* h, const float* img, const float* txt, float scale, const int32_t* lo, const int32_t* hi, int B, int C,
                     float* logits, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !img || !txt || !logits || B <= 0 || C <= 0 || ((lo == nullptr) != (hi == nullptr)))
    return fail(E, MVLPT_ERR_ARG, "logits_fwd: null/invalid argument");
  hipStream_t s = (hipStream_t)stream;
  const int e = E->arch.embed_dim;
  HeadRun& R = E->hrun = HeadRun();      // opened
  if (int rc = head_carve(E, "logits_fwd", B, C)) return rc;
  ProfScope ps(E, s, PC_HEAD, 2.0 * B * C * e, 4.0 * ((double)B * e + (double)C * e + (double)B * C));
  HIPCHK(E, launch_normalize_rows(img, R.imn, R.inorm, B, e, s));
  HIPCHK(E, launch_normalize_rows(txt, R.txn, R.tnorm, C, e, s));
  HIPCHK(E, launch_logits(R.imn, R.txn, scale, lo, hi, logits, B, C, e, s));
  R.B = B; R.C = C; R.scale = scale; R.lo = lo; R.hi = hi; R.kind = HeadKind::Plain;
  R.phase = Phase::Saved;
  return 0;
}

int mvlpt_logits_bwd(void* h, const float* dlogits, float* dimg, float* dtxt, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !dlogits) return fail(E, MVLPT_ERR_ARG, "logits_bwd: null argument");
  const HeadRun& R = E->hrun;
  if (R.phase != Phase::Saved || R.kind != HeadKind::Plain) return fail(E, MVLPT_ERR_STATE, "logits_bwd: call logits_fwd first");
  hipStream_t s = (hipStream_t)stream;
  const int e = E->arch.embed_dim;
  ProfScope ps(E, s, PC_HEAD, 4.0 * R.B * R.C * e, 4.0 * ((double)R.B * e + (double)R.C * e + (double)R.B * R.C) * 2);
  HIPCHK(E, launch_logits_bwd(dlogits, R.imn, R.txn, R.inorm, R.tnorm, R.scale, R.lo, R.hi, dimg, dtxt, R.B, R.C, e, s));
  return 0;
}

// The ranged head (trainers/mvlpt.py:556-581): image g against the text rows of its own class range, 0 outside it.  Every range
// [0, C) is CoCoOp's head (trainers/cocoop.py:184-189): image g against its own C text features txt[g*C .. g*C + C)
int mvlpt_logits_ranged_fwd(void* h, const float* img, const float* txt, float scale, const int32_t* class_lo, const int32_t* class_hi,
                            int G, int C, float* logits, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !img || !txt || !class_lo || !class_hi || !logits || G <= 0 || C <= 0 || G > 65535 || (int64_t)G * C > INT32_MAX)
    return fail(E, MVLPT_ERR_ARG, "logits_ranged_fwd: null/invalid argument");
  HeadRun& R = E->hrun = HeadRun();      // opened
  const int S = (int)build_range_table(class_lo, class_hi, G, C, E->h_range_host);      // (at most G * C)
  if (S <= 0) return fail(E, MVLPT_ERR_ARG, "logits_ranged_fwd: a class range is not inside [0, C], or every range is empty");
  hipStream_t s = (hipStream_t)stream;
  const int e = E->arch.embed_dim;
  const size_t ints = E->h_range_host.size();
  int32_t* tab = nullptr;
  if (int rc = head_carve(E, "logits_ranged_fwd", G, S, ints, &tab)) return rc;
  ProfScope ps(E, s, PC_HEAD, 2.0 * S * e, 4.0 * ((double)G * e + (double)S * e + (double)G * C));
  HIPCHK(E, hipMemcpyAsync(tab, E->h_range_host.data(), ints * 4, hipMemcpyHostToDevice, s));
  HIPCHK(E, launch_normalize_rows(img, R.imn, R.inorm, G, e, s));
  HIPCHK(E, launch_normalize_rows(txt, R.txn, R.tnorm, S, e, s));
  HIPCHK(E, launch_logits_ranged(R.imn, R.txn, scale, tab, tab + G, logits, G, C, e, s));
  R.B = G; R.C = C; R.S = S; R.scale = scale; R.kind = HeadKind::Ranged;
  R.rlo = tab; R.rstart = tab + G; R.rgrp = tab + 2 * G + 1 + S;
  R.phase = Phase::Saved;
  return 0;
}

// dtxt [S, e] and / or dimg [G, e] of the last mvlpt_logits_ranged_fwd (a null output's kernel is not launched)
int mvlpt_logits_ranged_bwd(void* h, const float* dlogits, float* dtxt, float* dimg, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !dlogits || (!dtxt && !dimg)) return fail(E, MVLPT_ERR_ARG, "logits_ranged_bwd: null argument");
  const HeadRun& R = E->hrun;
  if (R.phase != Phase::Saved || R.kind != HeadKind::Ranged) return fail(E, MVLPT_ERR_STATE, "logits_ranged_bwd: call logits_ranged_fwd first");
  hipStream_t s = (hipStream_t)stream;
  const int e = E->arch.embed_dim;
  ProfScope ps(E, s, PC_HEAD, 6.0 * R.S * e, 4.0 * ((double)R.B * e * 2 + 3.0 * R.S * e + (double)R.S));
  HIPCHK(E, launch_logits_ranged_bwd(dlogits, R.imn, R.txn, R.inorm, R.tnorm, R.scale, R.rlo, R.rstart, R.rgrp, dimg, dtxt, R.B, R.S, R.C, e, s));
  return 0;
}

int mvlpt_cross_entropy(void* h, const float* logits, const void* labels, int kind, int B, int C, float* loss, float* dlogits,
                        float* ncorrect, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E || !logits || !labels || !loss || B <= 0 || C <= 0 || (kind != 0 && kind != 1))
    return fail(E, MVLPT_ERR_ARG, "cross_entropy: null/invalid argument");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(E, E->ce_ws.reserve((size_t)2 * B * 4 + 256));
  ProfScope ps(E, s, PC_HEAD, 8.0 * B * C, 4.0 * 3.0 * B * C);
  HIPCHK(E, launch_cross_entropy(logits, labels, kind, B, C, (float*)E->ce_ws.p, loss, dlogits, ncorrect, s));
  return 0;
}

// ------------------------------------------------------------------------------------------------ kernel-level ops
#define OPCHK(call) HIPCHK(nullptr, call)

#if defined(MVLPT_GEMM_TRACE) || defined(MVLPT_ATTN_TRACE)
// debug builds: the timeline of one workgroup.  A zeroed device buffer of int64 records for the launch that follows, when the
// environment variable names a file (ptr() is null otherwise); dump() waits for the stream and writes the records to that file.
struct TraceCapture {
  const char* path; hipStream_t s; size_t bytes; DevBuf buf; hipError_t err = hipSuccess;
  TraceCapture(const char* env, size_t records, hipStream_t s_) : path(getenv(env)), s(s_), bytes(records * sizeof(long long)) {
    if (!path) return;
    err = buf.reserve(bytes);
    if (err == hipSuccess) err = hipMemsetAsync(buf.p, 0, bytes, s);
  }
  long long* ptr() const { return (long long*)buf.p; }
  hipError_t dump() {
    if (!path) return hipSuccess;
    std::vector<long long> h(bytes / sizeof(long long));
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(h.data(), buf.p, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    if (FILE* f = fopen(path, "wb")) { fwrite(h.data(), 1, bytes, f); fclose(f); }
    return hipSuccess;
  }
};
#endif

int mvlpt_op_gemm(int dtype, int epi, const void* A, const void* Bt, int M, int N, int K, const float* bias, const void* aux,
                  const float* resid, void* out, void* out2, mvlpt_stream_t stream) {
  GemmArgs g{A, Bt, M, N, K, bias, aux, resid, out, out2};
#ifdef MVLPT_GEMM_TRACE
  // debug builds: row pitches of A / Bt from the environment (tools/pitch_probe.py allocates the operands that wide)
  if (getenv("MVLPT_DBG_LDA")) g.lda = atoi(getenv("MVLPT_DBG_LDA"));
  if (getenv("MVLPT_DBG_LDB")) g.ldb = atoi(getenv("MVLPT_DBG_LDB"));
  // timeline of workgroup 0 -> $MVLPT_GEMM_TRACE_FILE (8 waves x 2048 int64 records)
  TraceCapture tc("MVLPT_GEMM_TRACE_FILE", 16 * 2048, (hipStream_t)stream);
  OPCHK(tc.err);
  g.trace = tc.ptr();
#endif
  OPCHK(launch_gemm(dtype, epi, g, (hipStream_t)stream));
#ifdef MVLPT_GEMM_TRACE
  OPCHK(tc.dump());
#endif
  return 0;
}
// every GemmArgs field the towers set, straight into launch_gemm (which checks them); the split and mixed entries below are this one
// with their fields preset
int mvlpt_op_gemm_ex(int dtype, int epi, const void* A, const void* Bt, int M, int N, int K, const float* bias, const void* aux,
                     const float* resid, void* out, void* out2, int a_split, int lda, int ldo, int ldb, int w8_exp, int out_lo8,
                     mvlpt_stream_t stream) {
  GemmArgs g{A, Bt, M, N, K, bias, aux, resid, out, out2};
  g.a_split = a_split; g.lda = lda; g.ldo = ldo; g.ldb = ldb; g.w8_exp = w8_exp; g.out_lo8 = out_lo8;
  OPCHK(launch_gemm(dtype, epi, g, (hipStream_t)stream));
  return 0;
}
// ---- stand-alone activation, kernel level (the launches mlp_up / mlp_up_bwd make under MVLPT_ACT_GELU)
static int op_activation(const char* who, bool bwd, int dtype, int act, ActArgs a, mvlpt_stream_t stream) {
  if (const char* why = act_check(dtype, act, bwd, a)) return fail(nullptr, MVLPT_ERR_ARG, std::string(who) + ": " + why);
  OPCHK(bwd ? launch_act_bwd(dtype, act, a, (hipStream_t)stream) : launch_act_fwd(dtype, act, a, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_activation_fwd(int dtype, int act, const float* u32, int ld_in, int M, int N, int out_format, void* out, int ld_out,
                            void* u16_out, mvlpt_stream_t stream) {
  return op_activation("op_activation_fwd", false, dtype, act, ActArgs{u32, ld_in, out, out_format, ld_out, u16_out, M, N}, stream);
}
int mvlpt_op_activation_bwd(int dtype, int act, const float* da32, int ld_in, const void* u16, int M, int N, int out_format, void* out,
                            int ld_out, mvlpt_stream_t stream) {
  return op_activation("op_activation_bwd", true, dtype, act, ActArgs{da32, ld_in, out, out_format, ld_out, const_cast<void*>(u16), M, N}, stream);
}
int mvlpt_op_gemm_route(int dtype, int epi, int a_split, int M, int N, int K, int fold_ntp, mvlpt_stream_t stream, int* tile_m,
                        int* tile_n, int* ring) {
  GemmArgs g{nullptr, nullptr, M, N, K, nullptr, nullptr, nullptr, nullptr, nullptr};
  g.a_split = a_split; g.fold_ntp = fold_ntp;
  GemmRoute r;
  if (gemm_route(dtype, epi, g, fold_ntp > 0, (hipStream_t)stream, &r) != hipSuccess) return fail(nullptr, MVLPT_ERR_ARG, "gemm_route: no kernel for this problem");
  if (tile_m) *tile_m = r.tile_m;
  if (tile_n) *tile_n = r.tile_n;
  if (ring) *ring = r.ring;
  return r.family;
}
int mvlpt_op_gemm_split(int dtype, int epi, const void* A, const void* Bt, int M, int N, int K, const float* bias, const void* aux,
                        const float* resid, void* out, void* out2, mvlpt_stream_t stream) {
  return mvlpt_op_gemm_ex(dtype, epi, A, Bt, M, N, K, bias, aux, resid, out, out2, 1, 0, 0, 0, 0, 0, stream);
}
// ---- mixed pair (GemmArgs::a_split == 2): [hi (cols x 16 bit) | residual bytes (cols, e5m2) | unused], pitch 2*cols elements
int mvlpt_op_pack_weight_mixed(int dtype, const float* w32, int rows, int cols, int transposed, void* out, int* w8_exp,
                               mvlpt_stream_t stream) {
  if (!w32 || !out || !w8_exp || rows <= 0 || cols <= 0) return fail(nullptr, MVLPT_ERR_ARG, "pack_weight_mixed: null/invalid argument");
  hipStream_t s = (hipStream_t)stream;
  const int K = transposed ? rows : cols, ld = K + K / 2;
  DevBuf scale;
  OPCHK(scale.reserve(16));
  float* sc = (float*)scale.p;
  if (transposed) OPCHK(launch_pack_weight_t(dtype, w32, out, rows, cols, s, ld));
  else OPCHK(launch_pack_weight(dtype, w32, out, rows, cols, ld, s));
  OPCHK(launch_grad_scale(w32, (size_t)rows * cols, 128.0f, sc, s));
  OPCHK(launch_pack_weight8(w32, (uint8_t*)out + (size_t)K * 2, rows, cols, transposed, K, (size_t)ld * 2, sc, s));
  float h = 1.0f;
  OPCHK(hipMemcpyAsync(&h, sc, 4, hipMemcpyDeviceToHost, s));
  OPCHK(hipStreamSynchronize(s));
  int e = 0; (void)frexpf(h, &e);
  *w8_exp = e - 1;
  return 0;
}
int mvlpt_op_gemm_mixed(int dtype, int epi, const void* A, const void* Bt, int ldb, int w8_exp, int M, int N, int K, const float* bias,
                        const void* aux, const float* resid, void* out, void* out2, mvlpt_stream_t stream) {
  const int out_lo8 = (epi == EPI_GELU_SPLIT || epi == EPI_GELUBWD_SPLIT) ? 1 : 0;
  return mvlpt_op_gemm_ex(dtype, epi, A, Bt, M, N, K, bias, aux, resid, out, out2, 2, 0, 0, ldb, w8_exp, out_lo8, stream);
}
// ---- LayerNorm folding, kernel level (the same launches block_fwd makes)
int mvlpt_op_fold_vectors(int dtype, const void* W16, int ld, const float* gamma, const float* beta, const float* b, float* colsum,
                          float* bias2, int N, int K, mvlpt_stream_t stream) {
  OPCHK(launch_fold_vectors(dtype, W16, ld, gamma, beta, b, colsum, bias2, N, K, (hipStream_t)stream));
  return 0;
}
// a LayerNorm-producing GEMM (g.ln_part / g.ln_ntp set): whole N tiles, and a slot per block of 128 columns; *nt: the slots it fills
static int op_gemm_producer(const char* who, int dtype, int epi, const GemmArgs& g, int* nt, mvlpt_stream_t stream) {
  const int bn = gemm_tile_n(dtype, epi, g, (hipStream_t)stream);
  if (bn <= 0 || g.N % bn || g.N / 128 > g.ln_ntp) return fail(nullptr, MVLPT_ERR_ARG, std::string(who) + ": ntp smaller than N / 128");
  if (nt) *nt = g.N / 128;
  OPCHK(launch_gemm(dtype, epi, g, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_gemm_ln_producer(int dtype, const void* A, int a_split, const void* Bt, int ldb, int w8_exp, int M, int N, int K,
                              const float* bias, const float* resid, const float* gamma, int x16_split, float* out32, void* x16,
                              float* part, int ntp, int* nt, mvlpt_stream_t stream) {
  GemmArgs g{A, Bt, M, N, K, bias, nullptr, resid, out32, nullptr};
  g.a_split = a_split; g.ldb = ldb; g.w8_exp = w8_exp;
  g.ln_gamma = gamma; g.ln_x16 = x16; g.ln_split = x16_split; g.ln_part = part; g.ln_ntp = ntp;
  return op_gemm_producer("gemm_ln_producer", dtype, EPI_RESID32_LN, g, nt, stream);
}
int mvlpt_op_gemm_folded(int dtype, int epi, const void* A16, int a_split, const void* Bt, int ldb, int w8_exp, int M, int N, int K,
                         const float* colsum, const float* bias2, const float* part, int ntp, int nt, void* out, void* out2,
                         mvlpt_stream_t stream) {
  GemmArgs g{A16, Bt, M, N, K, bias2, nullptr, nullptr, out, out2};
  g.a_split = a_split; g.ldb = ldb; g.w8_exp = w8_exp;
  g.out_lo8 = (a_split == 2 && epi == EPI_GELU_SPLIT) ? 1 : 0;
  g.fold_part = part; g.fold_colsum = colsum; g.fold_ntp = ntp; g.fold_nt = nt;
  OPCHK(launch_gemm(dtype, epi, g, (hipStream_t)stream));
  return 0;
}
// ---- packed residual stream, kernel level (the same launches block_fwd_packed makes)
int mvlpt_op_fold_weight(const void* W16, int ld, const float* gamma, void* Wg16, int ldg, float* colsum, int N, int K, mvlpt_stream_t stream) {
  OPCHK(launch_fold_weight(W16, ld, gamma, Wg16, ldg, colsum, N, K, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_respk_pack(const float* x, void* hi, uint8_t* lo, float* part, int ntp, int rows, int d, mvlpt_stream_t stream) {
  OPCHK(launch_respk_pack_rows(x, hi, lo, part, ntp, rows, d, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_assemble_packed(const float* patch_emb, const float* cls, const float* pos, const float* ln_g, const float* ln_b, void* hi,
                             uint8_t* lo, float* part, int ntp, int batch, int grid2, int d, mvlpt_stream_t stream) {
  OPCHK(launch_assemble_tokens_packed(patch_emb, cls, pos, ln_g, ln_b, hi, lo, part, ntp, batch, grid2, d, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_respk_unpack(const void* hi, const uint8_t* lo, int row_mul, float* out, int rows, int d, mvlpt_stream_t stream) {
  OPCHK(launch_respk_unpack_rows(hi, lo, row_mul, out, rows, d, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_gemm_residp(const void* A, const void* Bt, int ldb, int M, int N, int K, const float* bias, const void* hi_in,
                         const uint8_t* lo_in, void* hi_out, uint8_t* lo_out, float* part, int ntp, int* nt, mvlpt_stream_t stream) {
  GemmArgs g{A, Bt, M, N, K, bias, nullptr, nullptr, hi_out, nullptr};
  g.ldb = ldb;
  g.rp_hi_in = hi_in; g.rp_lo_in = lo_in; g.rp_lo_out = lo_out; g.ln_part = part; g.ln_ntp = ntp;
  return op_gemm_producer("gemm_residp", DT_F16, EPI_RESIDP_LN, g, nt, stream);
}
int mvlpt_op_cast_mixed(int dtype, const float* in, void* out, int64_t rows, int d, mvlpt_stream_t stream) {
  OPCHK(launch_cast_f32_split(dtype, in, out, (size_t)rows, d, nullptr, (hipStream_t)stream, 1));
  return 0;
}
// LayerNorm: every entry, old or _ex, fills the same arguments from (row_mul, split, dy_dtype); what a caller's arguments are
// checked against is each entry's own business
static int op_ln_fwd(int out_dtype, const float* x, int row_mul, const float* gamma, const float* beta, void* y, int rows, int d, int split,
                     mvlpt_stream_t stream) {
  LnFwdArgs a{x, nullptr, row_mul, gamma, beta, y, rows, d};
  a.split = split;
  OPCHK(launch_ln_fwd(out_dtype, a, (hipStream_t)stream));
  return 0;
}
static int op_ln_bwd(int dtype, const void* dy, int dy_dtype, const float* x, int row_mul, const float* gamma, const float* resid,
                     float* out32, void* out16, int rows, int d, int split, mvlpt_stream_t stream) {
  LnBwdArgs a{dy, dy_dtype, x, nullptr, row_mul, gamma, resid, out32, out16, rows, d};
  a.split = split;
  OPCHK(launch_ln_bwd(dtype, a, (hipStream_t)stream));
  return 0;
}
// pair-product attention (a.fmt 1: 16-bit pairs, 2: mixed pairs, hi + e5m2 residual byte).  Debug builds: timeline of one workgroup ->
// $MVLPT_ATTN_TRACE_FILE (8 waves x 256 int64 records)
static int op_attn32_fwd(int dtype, AttnArgs a, mvlpt_stream_t stream) {
#ifdef MVLPT_ATTN_TRACE
  TraceCapture tc("MVLPT_ATTN_TRACE_FILE", 8 * 256, (hipStream_t)stream);
  OPCHK(tc.err);
  a.trace = tc.ptr();
#endif
  OPCHK(launch_attn_fwd(dtype, a, (hipStream_t)stream));
#ifdef MVLPT_ATTN_TRACE
  OPCHK(tc.dump());
#endif
  return 0;
}
static int op_attn32_bwd(int dtype, AttnBwdArgs a, mvlpt_stream_t stream) {
#ifdef MVLPT_ATTN_TRACE
  TraceCapture tc("MVLPT_ATTN_TRACE_FILE", 8 * 256, (hipStream_t)stream);
  OPCHK(tc.err);
  a.trace = tc.ptr();
#endif
  OPCHK(launch_attn_bwd(dtype, a, (hipStream_t)stream));
#ifdef MVLPT_ATTN_TRACE
  OPCHK(tc.dump());
#endif
  return 0;
}
int mvlpt_op_layernorm_fwd_mixed(int out_dtype, const float* x, const float* gamma, const float* beta, void* y, int rows, int d,
                                 mvlpt_stream_t stream) {
  if (out_dtype == DT_F32) return fail(nullptr, MVLPT_ERR_ARG, "layernorm_fwd_mixed: 16-bit output only");
  return op_ln_fwd(out_dtype, x, 1, gamma, beta, y, rows, d, 2, stream);
}
int mvlpt_op_layernorm_bwd_mixed(int dtype, const void* dy, const float* x, const float* gamma, const float* resid, float* out32,
                                 void* out16, int rows, int d, mvlpt_stream_t stream) {
  return op_ln_bwd(dtype, dy, DT_F32, x, 1, gamma, resid, out32, out16, rows, d, 2, stream);
}
int mvlpt_op_attention32_fwd_mixed(int dtype, const void* qkv, void* out, float* lse, int N, int L, int H, int causal, int q_rows,
                                   mvlpt_stream_t stream) {
  AttnArgs a{qkv, out, lse, N, L, H, causal, q_rows};
  a.fmt = 2;
  return op_attn32_fwd(dtype, a, stream);
}
int mvlpt_op_attention32_bwd_mixed(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                                   void* dqkv, int N, int L, int H, int causal, mvlpt_stream_t stream) {
  AttnBwdArgs a{qkv, out, dout, lse, delta, dqkv, N, L, H, causal};
  a.fmt = 2;
  return op_attn32_bwd(dtype, a, stream);
}
int mvlpt_op_layernorm_fwd_split(int out_dtype, const float* x, const float* gamma, const float* beta, void* y, int rows, int d,
                                 mvlpt_stream_t stream) {
  if (out_dtype == DT_F32) return fail(nullptr, MVLPT_ERR_ARG, "layernorm_fwd_split: 16-bit output only");
  return op_ln_fwd(out_dtype, x, 1, gamma, beta, y, rows, d, 1, stream);
}
int mvlpt_op_layernorm_bwd_split(int dtype, const void* dy, const float* x, const float* gamma, const float* resid, float* out32,
                                 void* out16, int rows, int d, mvlpt_stream_t stream) {
  return op_ln_bwd(dtype, dy, DT_F32, x, 1, gamma, resid, out32, out16, rows, d, 1, stream);
}
int mvlpt_op_attention32_fwd(int dtype, const void* qkv, void* out, float* lse, int N, int L, int H, int causal, int q_rows,
                             mvlpt_stream_t stream) {
  AttnArgs a{qkv, out, lse, N, L, H, causal, q_rows};
  a.fmt = 1;
  return op_attn32_fwd(dtype, a, stream);
}
int mvlpt_op_attention32_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                             void* dqkv, int N, int L, int H, int causal, mvlpt_stream_t stream) {
  AttnBwdArgs a{qkv, out, dout, lse, delta, dqkv, N, L, H, causal};
  a.fmt = 1;
  return op_attn32_bwd(dtype, a, stream);
}
// ---- the text backward's launches under a gradient length (mvlpt_set_text_grad_len): saved operands at the pitch seq_pitch, read
// through the row map r -> (r / grad_len) * seq_pitch + r % grad_len; everything else compact.  The launchers check the maps.
int mvlpt_op_gemm_gelubwd_rows(int dtype, int epi, const void* A, const void* Bt, int M, int N, int K, const void* aux, void* out, int a_split,
                               int lda, int ldo, int ldb, int w8_exp, int out_lo8, int grad_len, int seq_pitch, mvlpt_stream_t stream) {
  if (epi != EPI_GELUBWD && epi != EPI_GELUBWD_SPLIT) return fail(nullptr, MVLPT_ERR_ARG, "op_gemm_gelubwd_rows: a GELU-backward epilogue");
  GemmArgs g{A, Bt, M, N, K, nullptr, aux, nullptr, out, nullptr};
  g.a_split = a_split; g.lda = lda; g.ldo = ldo; g.ldb = ldb; g.w8_exp = w8_exp; g.out_lo8 = out_lo8;
  g.aux_rows = RowMap{grad_len, seq_pitch};
  OPCHK(launch_gemm(dtype, epi, g, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_layernorm_bwd_rows(int dtype, const void* dy, int dy_dtype, const float* x, const float* gamma, const float* resid,
                                float* out32, void* out16, int rows, int d, int split, int grad_len, int seq_pitch, mvlpt_stream_t stream) {
  if (!dy || !x || !gamma || !out32 || rows <= 0 || grad_len <= 0 || rows % grad_len)
    return fail(nullptr, MVLPT_ERR_ARG, "op_layernorm_bwd_rows: null/invalid argument");
  LnBwdArgs a{dy, dy_dtype, x, nullptr, 1, gamma, resid, out32, out16, rows, d};
  a.split = split; a.x_rows = RowMap{grad_len, seq_pitch};
  OPCHK(launch_ln_bwd(dtype, a, (hipStream_t)stream));
  return 0;
}
// causal; pair: attention32.hip (lo8: mixed pairs), else the single-operand kernels of attention.hip
int mvlpt_op_attention_bwd_rows(int dtype, int pair, int lo8, const void* qkv, const void* out, const void* dout, const float* lse,
                                float* delta, void* dqkv, int N, int grad_len, int seq_pitch, int H, mvlpt_stream_t stream) {
  if (!qkv || !out || !dout || !lse || !delta || !dqkv) return fail(nullptr, MVLPT_ERR_ARG, "op_attention_bwd_rows: null argument");
  AttnBwdArgs a{qkv, out, dout, lse, delta, dqkv, N, grad_len, H, 1};
  a.Ls = seq_pitch; a.fmt = pair ? (lo8 ? 2 : 1) : 0;
  OPCHK(launch_attn_bwd(dtype, a, (hipStream_t)stream));
  return 0;
}
// ---- the pair attention under a shared prefix (mvlpt_set_text_shared_prefix; kernels.h AttnArgs::prefix): causal, slots
int mvlpt_op_attention32_fwd_prefix(int dtype, int lo8, const void* qkv, void* out, float* lse, int N, int L, int H, int prefix,
                                    mvlpt_stream_t stream) {
  if (!qkv || !out || prefix <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_attention32_fwd_prefix: null/invalid argument");
  AttnArgs a{qkv, out, lse, N, L, H, 1, 0};
  a.fmt = lo8 ? 2 : 1; a.prefix = prefix;
  OPCHK(launch_attn_fwd(dtype, a, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_attention32_bwd_prefix(int dtype, int lo8, const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                                    void* dqkv, float* kv_part, float part_mul, int N, int grad_len, int seq_len, int H, int prefix,
                                    mvlpt_stream_t stream) {
  if (!qkv || !out || !dout || !lse || !delta || !dqkv || !kv_part || prefix <= 0 || seq_len < grad_len)
    return fail(nullptr, MVLPT_ERR_ARG, "op_attention32_bwd_prefix: null/invalid argument");
  AttnBwdArgs a{qkv, out, dout, lse, delta, dqkv, N, grad_len, H, 1};
  a.fmt = lo8 ? 2 : 1; a.Ls = seq_len; a.prefix = prefix; a.kv_part = kv_part; a.part_mul = part_mul;
  OPCHK(launch_attn_bwd(dtype, a, (hipStream_t)stream));
  return 0;
}
// ... and the single-operand attention (attention.hip) under a shared prefix: the fast mode's kernels, same slots, 16-bit tensors
int mvlpt_op_attention_fwd_prefix(int dtype, const void* qkv, void* out, float* lse, int N, int L, int H, int prefix, mvlpt_stream_t stream) {
  if (!qkv || !out || prefix <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_attention_fwd_prefix: null/invalid argument");
  AttnArgs a{qkv, out, lse, N, L, H, 1};
  a.prefix = prefix;
  OPCHK(launch_attn_fwd(dtype, a, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_attention_bwd_prefix(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                                  float* kv_part, float part_mul, int N, int grad_len, int seq_len, int H, int prefix, mvlpt_stream_t stream) {
  if (!qkv || !out || !dout || !lse || !delta || !dqkv || !kv_part || prefix <= 0 || seq_len < grad_len)
    return fail(nullptr, MVLPT_ERR_ARG, "op_attention_bwd_prefix: null/invalid argument");
  AttnBwdArgs a{qkv, out, dout, lse, delta, dqkv, N, grad_len, H, 1};
  a.Ls = seq_len; a.prefix = prefix; a.kv_part = kv_part; a.part_mul = part_mul;
  OPCHK(launch_attn_bwd(dtype, a, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_layernorm_fwd(int out_dtype, const float* x, const float* gamma, const float* beta, void* y, int rows, int d,
                           mvlpt_stream_t stream) {
  return op_ln_fwd(out_dtype, x, 1, gamma, beta, y, rows, d, 0, stream);
}
int mvlpt_op_layernorm_bwd(int dtype, const void* dy, const float* x, const float* gamma, const float* resid, float* out32,
                           void* out16, int rows, int d, mvlpt_stream_t stream) {
  return op_ln_bwd(dtype, dy, dtype, x, 1, gamma, resid, out32, out16, rows, d, 0, stream);
}
int mvlpt_op_attention_fwd(int dtype, const void* qkv, void* out, float* lse, int N, int L, int H, int causal,
                           mvlpt_stream_t stream) {
  AttnArgs a{qkv, out, lse, N, L, H, causal};
  OPCHK(launch_attn_fwd(dtype, a, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_attention_wide_fwd(int dtype, const void* qkv, void* out, float* lse, int N, int L, int H, int head_width, int q_rows,
                                mvlpt_stream_t stream) {
  if (!attn_wide_supported(head_width)) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "op_attention_wide_fwd: head_width must be 80, 96, 112 or 128");
  if (!qkv || !out || N <= 0 || L <= 0 || H <= 0 || q_rows < 0 || (dtype != DT_F16 && dtype != DT_BF16))
    return fail(nullptr, MVLPT_ERR_ARG, "op_attention_wide_fwd: null / invalid argument");
  AttnArgs a{qkv, out, lse, N, L, H, 0, q_rows};
  OPCHK(launch_attn_fwd_wide(dtype, a, head_width, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_attention_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                           void* dqkv, int N, int L, int H, int causal, mvlpt_stream_t stream) {
  AttnBwdArgs a{qkv, out, dout, lse, delta, dqkv, N, L, H, causal};
  OPCHK(launch_attn_bwd(dtype, a, (hipStream_t)stream));
  return 0;
}
// ---- the convolutional tower at kernel level
int mvlpt_op_pack_conv_weight(const float* w32, int Cout, int Cin, int k, int cin_pad, void* out, int* kp, mvlpt_stream_t stream) {
  if (Cout <= 0 || Cin <= 0 || cin_pad < Cin || cin_pad % 8) return fail(nullptr, MVLPT_ERR_ARG, "op_pack_conv_weight: Cout, Cin > 0, cin_pad >= Cin, cin_pad % 8 == 0");
  if (k != 1 && k != 3) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "op_pack_conv_weight: kernel size must be 1 or 3");
  if (kp) *kp = conv_kp(k, cin_pad);
  if (!out) return kp ? 0 : fail(nullptr, MVLPT_ERR_ARG, "op_pack_conv_weight: null pointer");
  if (!w32) return fail(nullptr, MVLPT_ERR_ARG, "op_pack_conv_weight: null pointer");
  OPCHK(launch_pack_conv_weight(w32, out, Cout, Cin, k, cin_pad, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_conv2d(const void* x, const void* w, const float* scale, const float* shift, const void* resid, void* y, int B, int H,
                    int W, int Cin, int Cout, int k, int stride, int relu, mvlpt_stream_t stream) {
  ConvArgs a{x, w, scale, shift, resid, y, B, H, W, Cin, Cout, k, stride, relu};
  if (const char* why = conv2d_check(a)) {
    const bool arg = !x || !w || !scale || !shift || !y || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0;
    return fail(nullptr, arg ? MVLPT_ERR_ARG : MVLPT_ERR_UNSUPPORTED, std::string("op_conv2d: ") + why);
  }
  OPCHK(launch_conv2d(a, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_avgpool2x2(const void* x, void* y, int B, int H, int W, int C, mvlpt_stream_t stream) {
  if (!x || !y || B <= 0 || H < 2 || W < 2 || C <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_avgpool2x2: null pointer or empty map");
  if (C % 8) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "op_avgpool2x2: C must be a multiple of 8");
  OPCHK(launch_avgpool2x2(x, y, B, H, W, C, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_nchw_to_nhwc8(const void* image, int image_dtype, void* out, int B, int R, mvlpt_stream_t stream) {
  if (!image || !out || B <= 0 || R <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_nchw_to_nhwc8: null pointer or empty image");
  if (image_dtype != MVLPT_DT_F32 && image_dtype != MVLPT_DT_F16 && image_dtype != MVLPT_DT_BF16) return fail(nullptr, MVLPT_ERR_ARG, "op_nchw_to_nhwc8: unknown image dtype");
  OPCHK(launch_nchw_to_nhwc8(image, image_dtype, out, B, R, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_attnpool_tokens(const void* x, const float* pos, void* tok, int B, int HW, int E, mvlpt_stream_t stream) {
  if (!x || !pos || !tok || B <= 0 || B > 65535 || HW <= 0 || E <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_attnpool_tokens: null pointer or extent out of range");
  OPCHK(launch_attnpool_tokens(x, pos, tok, B, HW, E, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_attnpool_query(const void* q, const void* kv, void* out, int B, int T, int E, mvlpt_stream_t stream) {
  if (!q || !kv || !out || B <= 0 || B > 65535 || T <= 0 || E <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_attnpool_query: null pointer or extent out of range");
  if (T > attnpool_max_tokens() || E % 64) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "op_attnpool_query: T <= 145 and E % 64 == 0");
  OPCHK(launch_attnpool_query(q, kv, out, B, T, E, (hipStream_t)stream));
  return 0;
}

int mvlpt_op_cast(int dtype, const float* in, void* out, int64_t n, mvlpt_stream_t stream) {
  OPCHK(launch_cast_f32_to16(dtype, in, out, (size_t)n, nullptr, (hipStream_t)stream));
  return 0;
}
// ---- LayerNorm, the operand-format kernels and the patch extraction with every argument the towers set; everything is checked here,
// before a launch, so that a refused call leaves its output untouched
static bool is16(int dt) { return dt == DT_F16 || dt == DT_BF16; }
static int ln_shape_check(const char* who, int rows, int d, int row_mul, int split) {
  if (rows < 0 || d <= 0 || row_mul < 1 || split < 0 || split > 2) return fail(nullptr, MVLPT_ERR_ARG, std::string(who) + ": rows >= 0, d > 0, row_mul >= 1, split in {0, 1, 2}");
  if (d % 4 || d > 2048) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, std::string(who) + ": d must be a multiple of 4 and at most 2048");
  return 0;
}
int mvlpt_op_layernorm_fwd_ex(int out_dtype, const float* x, int row_mul, const float* gamma, const float* beta, void* y, int rows, int d,
                              int split, mvlpt_stream_t stream) {
  if (!x || !gamma || !beta || !y) return fail(nullptr, MVLPT_ERR_ARG, "op_layernorm_fwd_ex: null pointer");
  if (out_dtype != DT_F32 && !is16(out_dtype)) return fail(nullptr, MVLPT_ERR_ARG, "op_layernorm_fwd_ex: unknown output dtype");
  if (out_dtype == DT_F32 && split) return fail(nullptr, MVLPT_ERR_ARG, "op_layernorm_fwd_ex: a pair output is 16-bit");
  if (int rc = ln_shape_check("op_layernorm_fwd_ex", rows, d, row_mul, split)) return rc;
  return op_ln_fwd(out_dtype, x, row_mul, gamma, beta, y, rows, d, split, stream);
}
int mvlpt_op_layernorm_bwd_ex(int dtype, const void* dy, int dy_dtype, const float* x, int row_mul, const float* gamma, const float* resid,
                              float* out32, void* out16, int rows, int d, int split, mvlpt_stream_t stream) {
  if (!dy || !x || !gamma || !out32) return fail(nullptr, MVLPT_ERR_ARG, "op_layernorm_bwd_ex: null pointer");
  if (!is16(dtype) || (dy_dtype != DT_F32 && dy_dtype != dtype)) return fail(nullptr, MVLPT_ERR_ARG, "op_layernorm_bwd_ex: dtype is fp16 or bf16, dy_dtype fp32 or dtype");
  if (int rc = ln_shape_check("op_layernorm_bwd_ex", rows, d, row_mul, split)) return rc;
  return op_ln_bwd(dtype, dy, dy_dtype, x, row_mul, gamma, resid, out32, out16, rows, d, split, stream);
}
int mvlpt_op_layernorm_route(int rows, int d, mvlpt_stream_t stream, int* nv, int* grid) {
  if (rows <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_layernorm_route: rows > 0 (an empty call launches nothing)");
  if (int rc = ln_shape_check("op_layernorm_route", rows, d, 1, 0)) return rc;
  const LnRoute r = ln_route(rows, d, (hipStream_t)stream);
  if (nv) *nv = r.nv;
  if (grid) *grid = r.grid;
  return r.stream;
}
int mvlpt_op_cast_ex(int dtype, const float* in, void* out, int64_t rows, int d, int format, const float* scale_dev, mvlpt_stream_t stream) {
  if (!in || !out) return fail(nullptr, MVLPT_ERR_ARG, "op_cast_ex: null pointer");
  if (!is16(dtype) || format < 0 || format > 2 || rows < 0 || d <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_cast_ex: dtype is fp16 or bf16, format in {0, 1, 2}, rows >= 0, d > 0");
  if (d % 4) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "op_cast_ex: d must be a multiple of 4");
  if (format == 0) OPCHK(launch_cast_f32_to16(dtype, in, out, (size_t)rows * d, scale_dev, (hipStream_t)stream));
  else OPCHK(launch_cast_f32_split(dtype, in, out, (size_t)rows, d, scale_dev, (hipStream_t)stream, format == 2));
  return 0;
}
int mvlpt_op_cast_to_f32(int in_dtype, const void* in, float* out, int64_t n, mvlpt_stream_t stream) {
  if (!in || !out || n < 0) return fail(nullptr, MVLPT_ERR_ARG, "op_cast_to_f32: null pointer or n < 0");
  if (in_dtype != DT_F32 && !is16(in_dtype)) return fail(nullptr, MVLPT_ERR_ARG, "op_cast_to_f32: unknown input dtype");
  OPCHK(launch_cast_any_to_f32(in_dtype, in, out, (size_t)n, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_pack_weight(int dtype, const float* w32, int rows, int cols, int transposed, int ld_out, void* out, mvlpt_stream_t stream) {
  if (!w32 || !out || rows <= 0 || cols <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_pack_weight: null pointer or empty weight");
  if (dtype != DT_F32 && !is16(dtype)) return fail(nullptr, MVLPT_ERR_ARG, "op_pack_weight: unknown dtype");
  const int width = transposed ? rows : cols;
  if (ld_out <= 0) ld_out = width;
  if (ld_out < width) return fail(nullptr, MVLPT_ERR_ARG, "op_pack_weight: ld_out is shorter than a row of the output");
  if (transposed) OPCHK(launch_pack_weight_t(dtype, w32, out, rows, cols, (hipStream_t)stream, ld_out));
  else OPCHK(launch_pack_weight(dtype, w32, out, rows, cols, ld_out, (hipStream_t)stream));
  return 0;
}
static int patchify_check(const char* who, int dtype, int image_dtype, int R, int P) {
  if (!is16(dtype) || (image_dtype != DT_F32 && !is16(image_dtype))) return fail(nullptr, MVLPT_ERR_ARG, std::string(who) + ": dtype is fp16 or bf16, image_dtype fp32, fp16 or bf16");
  if (R <= 0 || P <= 0) return fail(nullptr, MVLPT_ERR_ARG, std::string(who) + ": R, P > 0");
  if (R % P) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, std::string(who) + ": R must be a multiple of P");
  return 0;
}
int mvlpt_op_patchify(int dtype, const void* image, int image_dtype, void* out, int B, int R, int P, int Kp, mvlpt_stream_t stream) {
  if (!image || !out || B <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_patchify: null pointer or B <= 0");
  if (int rc = patchify_check("op_patchify", dtype, image_dtype, R, P)) return rc;
  if (Kp % 8) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "op_patchify: Kp must be a multiple of 8");
  if (Kp < 3 * P * P) return fail(nullptr, MVLPT_ERR_ARG, "op_patchify: Kp is shorter than a patch (3 P^2)");
  OPCHK(launch_patchify(dtype, image, image_dtype, out, B, R, P, Kp, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_patchify_route(int dtype, int image_dtype, int R, int P) {
  if (int rc = patchify_check("op_patchify_route", dtype, image_dtype, R, P)) return rc;
  return patchify_route(dtype, image_dtype, R, P);
}
// The ranged glue without a tower (tests).  The range table is built and checked on the host, uploaded into a temporary buffer, and the
// call waits for its kernel before the buffer is freed.
static int op_range_table(const int32_t* class_lo, const int32_t* class_hi, int G, int C, DevBuf& dev, int* S) {
  std::vector<int32_t> t;
  const int64_t S64 = build_range_table(class_lo, class_hi, G, C, t);
  if (S64 <= 0) return fail(nullptr, MVLPT_ERR_ARG, "ranged op: a class range is not inside [0, C], or every range is empty");
  *S = (int)S64;
  OPCHK(dev.reserve(t.size() * 4));
  OPCHK(hipMemcpy(dev.p, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  return 0;
}
int mvlpt_op_assemble_prompts_ranged(const float* prefix, const float* suffix, const float* ctx, int n_ctx, const int32_t* layout,
                                     const float* pos, float* x, const int32_t* class_lo, const int32_t* class_hi, int G, int C, int L,
                                     int d, mvlpt_stream_t stream) {
  if (!prefix || !suffix || !ctx || !layout || !pos || !x || !class_lo || !class_hi || G <= 0 || C <= 0 || L <= n_ctx + 1 || n_ctx <= 0 ||
      d <= 0)
    return fail(nullptr, MVLPT_ERR_ARG, "op_assemble_prompts_ranged: null/invalid argument");
  DevBuf table; int S = 0;
  if (int rc = op_range_table(class_lo, class_hi, G, C, table, &S)) return rc;
  const int32_t* dev = (const int32_t*)table.p;
  OPCHK(launch_assemble_prompts_ranged(prefix, suffix, ctx, n_ctx, layout, pos, x, dev + 2 * G + 1, dev + 2 * G + 1 + S, S, L, d,
                                       (hipStream_t)stream));
  OPCHK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}
int mvlpt_op_gather_ctx_grad_ranged(const float* dx, const int32_t* ctx_pos, const int32_t* class_lo, const int32_t* class_hi, int G, int C,
                                    int L, int d, int n_ctx, float* dctx, mvlpt_stream_t stream) {
  if (!dx || !ctx_pos || !dctx || !class_lo || !class_hi || G <= 0 || C <= 0 || L <= 0 || n_ctx <= 0 || d <= 0)
    return fail(nullptr, MVLPT_ERR_ARG, "op_gather_ctx_grad_ranged: null/invalid argument");
  DevBuf table; int S = 0;
  if (int rc = op_range_table(class_lo, class_hi, G, C, table, &S)) return rc;
  const int32_t* dev = (const int32_t*)table.p;
  OPCHK(launch_gather_ctx_grad_ranged(dx, ctx_pos, dev, dev + G, G, L, d, n_ctx, dctx, nullptr, (hipStream_t)stream));
  OPCHK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

// The dense head's neighbours and the fp32 glue without a tower (tests): the launchers the towers call, unchanged.
int mvlpt_op_sgemm_bt(const float* A, const float* Bt, float* Cm, int M, int N, int K, const float* alpha_dev, mvlpt_stream_t stream) {
  if (!A || !Bt || !Cm) return fail(nullptr, MVLPT_ERR_ARG, "op_sgemm_bt: null argument");
  OPCHK(launch_sgemm_bt(A, Bt, Cm, M, N, K, alpha_dev, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_grad_scale(const float* v, int64_t n, float target, float* scale_dev, mvlpt_stream_t stream) {
  if (!v || !scale_dev || n <= 0 || !(target > 0.f)) return fail(nullptr, MVLPT_ERR_ARG, "op_grad_scale: null/invalid argument");
  OPCHK(launch_grad_scale(v, (size_t)n, target, scale_dev, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_optim_step(const MvlptOptimHyper* hyper, float* param, const float* grad, float* state1, float* state2, int64_t n,
                        const MvlptOptimSeg* segs_dev, int n_segs, const float* loss_dev, int32_t* skipped_dev, mvlpt_stream_t stream) {
  if (!hyper || !param || !grad || !segs_dev || n <= 0 || n_segs <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_optim_step: null/invalid argument");
  const MvlptOptimHyper& h = *hyper;
  if (h.kind < MVLPT_OPTIM_SGD || h.kind > MVLPT_OPTIM_ADAMW || h.launch < 1) return fail(nullptr, MVLPT_ERR_ARG, "op_optim_step: unknown kind, or launch < 1");
  if (n_segs > MVLPT_OPTIM_MAX_SEGS) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "op_optim_step: more than MVLPT_OPTIM_MAX_SEGS segments");
  if ((h.kind == MVLPT_OPTIM_SGD && h.momentum != 0.0 && !state1) || (h.kind != MVLPT_OPTIM_SGD && (!state1 || !state2)))
    return fail(nullptr, MVLPT_ERR_ARG, "op_optim_step: this optimizer kind needs its state buffer(s)");
  if (h.kind == MVLPT_OPTIM_SGD && h.nesterov && (h.momentum <= 0.0 || h.dampening != 0.0))
    return fail(nullptr, MVLPT_ERR_ARG, "op_optim_step: nesterov needs a momentum and zero dampening");
  if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)state1 | (uintptr_t)state2) & 15) != 0)
    return fail(nullptr, MVLPT_ERR_ARG, "op_optim_step: the flat buffers must be 16-byte aligned");
  OPCHK(launch_optim_step(h, param, grad, state1, state2, n, segs_dev, n_segs, loss_dev, skipped_dev, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_reduce_prompt_rows(int dtype, float* dx32, void* dx16, int B, int L, int d, int row0, int n, float* out,
                                const float* scale_dev, int zero_after, int split16, const float* vmask, mvlpt_stream_t stream) {
  if (!dx32 || !out || B <= 0 || d <= 0 || n <= 0 || row0 < 0 || row0 + n > L || split16 < 0 || split16 > 2)
    return fail(nullptr, MVLPT_ERR_ARG, "op_reduce_prompt_rows: null/invalid argument");
  OPCHK(launch_reduce_prompt_rows(dtype, dx32, dx16, B, L, d, row0, n, out, scale_dev, zero_after, (hipStream_t)stream, split16, vmask));
  return 0;
}
int mvlpt_op_gather_ctx_grad(const float* dx, const int32_t* ctx_pos, int C, int L, int d, int n_ctx, int per_class, float* dctx,
                             const float* scale_dev, mvlpt_stream_t stream) {
  if (!dx || !ctx_pos || !dctx || C <= 0 || L <= 0 || n_ctx <= 0 || d <= 0)
    return fail(nullptr, MVLPT_ERR_ARG, "op_gather_ctx_grad: null/invalid argument");
  OPCHK(launch_gather_ctx_grad(dx, ctx_pos, C, L, d, n_ctx, per_class, dctx, scale_dev, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_overwrite_ctx_rows(const float* rows, const int32_t* ctx_pos, float* x, int C, int L, int d, int n_ctx, mvlpt_stream_t stream) {
  if (!rows || !ctx_pos || !x || C <= 0 || L <= 0 || n_ctx <= 0 || n_ctx > L || d <= 0 || d % 4)
    return fail(nullptr, MVLPT_ERR_ARG, "op_overwrite_ctx_rows: null/invalid argument");
  OPCHK(launch_overwrite_ctx_rows(rows, ctx_pos, x, C, L, d, n_ctx, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_gather_zero_ctx_grad(int dtype, float* dx32, void* dx16, int split16, const int32_t* ctx_pos, int C, int L, int d, int n_ctx,
                                  float* out, const float* scale_dev, mvlpt_stream_t stream) {
  if (!dx32 || !ctx_pos || !out || C <= 0 || L <= 0 || n_ctx <= 0 || n_ctx > L || d <= 0 || d % 4 || split16 < 0 || split16 > 2 ||
      (dtype != DT_F16 && dtype != DT_BF16))
    return fail(nullptr, MVLPT_ERR_ARG, "op_gather_zero_ctx_grad: null/invalid argument");
  OPCHK(launch_gather_zero_ctx_grad(dtype, dx32, dx16, split16, ctx_pos, C, L, d, n_ctx, out, scale_dev, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_attention_bwd_cls(int dtype, const void* qkv, const void* o_cls, const void* do_cls, const float* lse, void* dqkv, int N,
                               int L, int H, mvlpt_stream_t stream) {
  if (!qkv || !o_cls || !do_cls || !lse || !dqkv) return fail(nullptr, MVLPT_ERR_ARG, "op_attention_bwd_cls: null argument");
  OPCHK(launch_attn_bwd_cls(dtype, qkv, o_cls, do_cls, lse, dqkv, N, L, H, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_copy_rows(const void* src, void* dst, const int32_t* idx, int rows, int row_bytes, int scatter, mvlpt_stream_t stream) {
  if (!src || !dst || !idx || rows <= 0 || row_bytes <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_copy_rows: null/invalid argument");
  OPCHK(launch_copy_rows(src, dst, idx, rows, row_bytes, scatter, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_overwrite_rows(const float* rows, int n, float* x, int B, int L, int d, const float* vmask, mvlpt_stream_t stream) {
  if (!rows || !x || n <= 0 || B <= 0 || 1 + n > L || d <= 0 || d % 4)
    return fail(nullptr, MVLPT_ERR_ARG, "op_overwrite_rows: null/invalid argument");
  OPCHK(launch_overwrite_rows(rows, n, x, B, L, d, (hipStream_t)stream, vmask));
  return 0;
}
int mvlpt_op_assemble_tokens(const float* patch_emb, const float* cls, const float* pos, const float* ln_g, const float* ln_b,
                             const float* vpt, int n_vpt, const float* vmask, float* x, int B, int G2, int d, mvlpt_stream_t stream) {
  if (!patch_emb || !cls || !pos || !ln_g || !ln_b || !x || B <= 0 || G2 <= 0 || d <= 0 || n_vpt < 0 || (n_vpt > 0 && !vpt) ||
      (vmask && n_vpt == 0))
    return fail(nullptr, MVLPT_ERR_ARG, "op_assemble_tokens: null/invalid argument");
  OPCHK(launch_assemble_tokens(patch_emb, cls, pos, ln_g, ln_b, vpt, n_vpt, x, B, G2, d, (hipStream_t)stream, vmask));
  return 0;
}
int mvlpt_op_assemble_prompts(const float* prefix, const float* suffix, const float* ctx, int ctx_per_class, int n_ctx,
                              const int32_t* layout, const float* pos, const int32_t* eot, float* x, int32_t* ctx_pos, int32_t* eot_rows,
                              int C, int L, int d, mvlpt_stream_t stream) {
  if (!prefix || !suffix || !layout || !pos || !eot || !x || !eot_rows || C <= 0 || n_ctx < 0 || L < n_ctx + 1 || d <= 0 ||
      (n_ctx > 0 && (!ctx || !ctx_pos)))
    return fail(nullptr, MVLPT_ERR_ARG, "op_assemble_prompts: null/invalid argument");
  hipStream_t s = (hipStream_t)stream;
  OPCHK(launch_assemble_prompts(prefix, suffix, ctx, ctx_per_class, n_ctx, layout, pos, x, C, L, d, s));
  OPCHK(launch_eot_rows(eot, eot_rows, C, L, s));
  OPCHK(launch_build_ctx_pos(layout, ctx_pos, C, L, n_ctx, s));
  return 0;
}

// The zero-shot glue without a tower (tests): ids is a DEVICE int32 [S, ld] table here, and every id in columns 0 .. L-1 must be inside
// [0, vocab) — the caller's responsibility at this level (mvlpt_text_encode_tokens checks its host table).
int mvlpt_op_embed_tokens(const float* emb, const float* pos, const int32_t* ids, int ld, float* x, int S, int L, int d,
                          mvlpt_stream_t stream) {
  if (!emb || !pos || !ids || !x || S <= 0 || L <= 0 || ld < L || d <= 0 || d % 4)
    return fail(nullptr, MVLPT_ERR_ARG, "op_embed_tokens: null/invalid argument");
  OPCHK(launch_embed_tokens(emb, pos, ids, ld, x, S, L, d, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_ensemble_features(const float* feats, float* out, int T, int C, int e, mvlpt_stream_t stream) {
  if (!feats || !out || T <= 0 || C <= 0 || e <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_ensemble_features: null/invalid argument");
  OPCHK(launch_ensemble_features(feats, out, T, C, e, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_normalize_rows(const float* x, float* xn, float* norm, int rows, int d, mvlpt_stream_t stream) {
  if (!x || !xn || !norm || rows <= 0 || d <= 0) return fail(nullptr, MVLPT_ERR_ARG, "op_normalize_rows: null/invalid argument");
  OPCHK(launch_normalize_rows(x, xn, norm, rows, d, (hipStream_t)stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------ prompt interpretation
// Every limit of include/mvlpt_hip.h is checked here, before a launch: the kernels (nearest.hip) trust their arguments.
static int nearest_check(Engine* E, const char* who, int R, int V, int d, int k) {
  const std::string w = std::string(who) + ": ";
  if (R < 1 || V < 1) return fail(E, MVLPT_ERR_ARG, w + "R and V must be at least 1");
  if (k > MVLPT_NEAREST_MAX_K) return fail(E, MVLPT_ERR_UNSUPPORTED, w + "k exceeds MVLPT_NEAREST_MAX_K");
  if (k < 1 || k > V) return fail(E, MVLPT_ERR_ARG, w + "k must lie in [1, min(V, MVLPT_NEAREST_MAX_K)]");
  if (d < 4 || d % 4 || d > 1024) return fail(E, MVLPT_ERR_ARG, w + "d must be a multiple of 4 in [4, 1024]");
  if (R > MVLPT_NEAREST_MAX_ROWS) return fail(E, MVLPT_ERR_ARG, w + "R exceeds MVLPT_NEAREST_MAX_ROWS (chunk the rows)");
  return 0;
}
static int nearest_run(Engine* E, const char* who, const float* q, const float* table, int R, int V, int d, int k, int32_t* idx,
                       float* dist, void* ws, const NearestPlan& p, hipStream_t s) {
  if ((((uintptr_t)q | (uintptr_t)table) & 15) != 0) return fail(E, MVLPT_ERR_ARG, std::string(who) + ": q and table must be 16-byte aligned");
  const hipError_t e = launch_nearest_rows(q, table, R, V, d, k, idx, dist, ws, p, s);
  if (e != hipSuccess) return hipfail(E, e, who);
  return 0;
}
int mvlpt_nearest_workspace_bytes(int R, int V, int d, int k, mvlpt_stream_t stream, int64_t* out) {
  if (!out) return fail(nullptr, MVLPT_ERR_ARG, "nearest_workspace_bytes: null argument");
  if (int rc = nearest_check(nullptr, "nearest_workspace_bytes", R, V, d, k)) return rc;
  *out = (int64_t)nearest_plan(R, V, k, stream_cus((hipStream_t)stream)).ws_bytes;
  return 0;
}
int mvlpt_op_nearest_rows(const float* q, const float* table, int R, int V, int d, int k, int32_t* idx, float* dist, void* workspace,
                          int64_t workspace_bytes, mvlpt_stream_t stream) {
  if (!q || !table || !idx || !dist || !workspace) return fail(nullptr, MVLPT_ERR_ARG, "op_nearest_rows: null argument");
  if (int rc = nearest_check(nullptr, "op_nearest_rows", R, V, d, k)) return rc;
  const NearestPlan p = nearest_plan(R, V, k, stream_cus((hipStream_t)stream));
  if (workspace_bytes < 0 || (uint64_t)workspace_bytes < p.ws_bytes || ((uintptr_t)workspace & 7) != 0)
    return fail(nullptr, MVLPT_ERR_ARG, "op_nearest_rows: the workspace is smaller than mvlpt_nearest_workspace_bytes (" +
                                            std::to_string(p.ws_bytes) + " bytes), or not 8-byte aligned");
  return nearest_run(nullptr, "op_nearest_rows", q, table, R, V, d, k, idx, dist, workspace, p, (hipStream_t)stream);
}
int mvlpt_nearest_tokens(void* h, const float* q, int R, int k, int32_t* idx, float* dist, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  if (!q || !idx || !dist) return fail(E, MVLPT_ERR_ARG, "nearest_tokens: null argument");
  if (!E->tok_emb || E->vocab <= 0)
    return fail(E, MVLPT_ERR_STATE, "nearest_tokens: token_embedding.weight is not loaded (mvlpt_load_frozen)");
  if (int rc = nearest_check(E, "nearest_tokens", R, E->vocab, E->arch.text_width, k)) return rc;
  const NearestPlan p = nearest_plan(R, E->vocab, k, stream_cus((hipStream_t)stream));
  HIPCHK(E, E->near_ws.reserve(p.ws_bytes));
  return nearest_run(E, "nearest_tokens", q, E->tok_emb, R, E->vocab, E->arch.text_width, k, idx, dist, E->near_ws.p, p, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ test-time prompt tuning head
// Every limit of include/mvlpt_hip.h is checked here, before a launch: the kernels (tpt.hip) trust their arguments.
static int tpt_check(const char* who, int G, int V, int C, int e, int k) {
  const std::string w = std::string(who) + ": ";
  if (G < 1 || G > MVLPT_TPT_MAX_GROUPS) return fail(nullptr, MVLPT_ERR_ARG, w + "G must lie in [1, MVLPT_TPT_MAX_GROUPS]");
  if (V < 1 || V > MVLPT_TPT_MAX_VIEWS) return fail(nullptr, MVLPT_ERR_ARG, w + "V must lie in [1, MVLPT_TPT_MAX_VIEWS]");
  if (C < 1 || C > MVLPT_TPT_MAX_CLASSES) return fail(nullptr, MVLPT_ERR_ARG, w + "C must lie in [1, MVLPT_TPT_MAX_CLASSES]");
  if (e < 4 || e % 4 || e > 1024) return fail(nullptr, MVLPT_ERR_ARG, w + "e must be a multiple of 4 in [4, 1024]");
  if (k < 1 || k > V) return fail(nullptr, MVLPT_ERR_ARG, w + "k must lie in [1, V]");
  if ((int64_t)G * C >= ((int64_t)1 << 31)) return fail(nullptr, MVLPT_ERR_ARG, w + "G * C must stay below 2^31 (chunk the images)");
  return 0;
}
static int tpt_ws_check(const char* who, const void* ws, int64_t have, size_t need) {
  if (!ws || have < 0 || (uint64_t)have < need || ((uintptr_t)ws & 15) != 0)
    return fail(nullptr, MVLPT_ERR_ARG, std::string(who) + ": the workspace is smaller than mvlpt_tpt_workspace_bytes (" +
                                            std::to_string(need) + " bytes), or not 16-byte aligned");
  return 0;
}
int mvlpt_tpt_workspace_bytes(int G, int V, int C, int e, int k, int64_t* bytes) {
  if (!bytes) return fail(nullptr, MVLPT_ERR_ARG, "tpt_workspace_bytes: null argument");
  if (int rc = tpt_check("tpt_workspace_bytes", G, V, C, e, k)) return rc;
  *bytes = (int64_t)tpt_plan(G, V, C, e, k).ws_bytes;
  return 0;
}
int mvlpt_op_tpt_head_fwd(const float* img, const float* txt, float scale, int G, int V, int C, int e, int k, float* loss, float* H,
                          int32_t* sel, float* z, void* workspace, int64_t workspace_bytes, mvlpt_stream_t stream) {
  if (!img || !txt || !loss || !H || !sel) return fail(nullptr, MVLPT_ERR_ARG, "op_tpt_head_fwd: null argument");
  if (int rc = tpt_check("op_tpt_head_fwd", G, V, C, e, k)) return rc;
  if ((((uintptr_t)img | (uintptr_t)txt) & 15) != 0) return fail(nullptr, MVLPT_ERR_ARG, "op_tpt_head_fwd: img and txt must be 16-byte aligned");
  const TptPlan p = tpt_plan(G, V, C, e, k);
  if (int rc = tpt_ws_check("op_tpt_head_fwd", workspace, workspace_bytes, p.ws_bytes)) return rc;
  OPCHK(launch_tpt_head_fwd(img, txt, scale, G, V, C, e, k, loss, H, sel, z, workspace, p, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_tpt_head_bwd(const float* w, float scale, int G, int V, int C, int e, int k, float* dtxt, void* workspace,
                          int64_t workspace_bytes, mvlpt_stream_t stream) {
  if (!dtxt) return fail(nullptr, MVLPT_ERR_ARG, "op_tpt_head_bwd: null argument");
  if (int rc = tpt_check("op_tpt_head_bwd", G, V, C, e, k)) return rc;
  if (((uintptr_t)dtxt & 15) != 0) return fail(nullptr, MVLPT_ERR_ARG, "op_tpt_head_bwd: dtxt must be 16-byte aligned");
  const TptPlan p = tpt_plan(G, V, C, e, k);
  if (int rc = tpt_ws_check("op_tpt_head_bwd", workspace, workspace_bytes, p.ws_bytes)) return rc;
  OPCHK(launch_tpt_head_bwd(w, scale, G, V, C, e, k, dtxt, workspace, p, (hipStream_t)stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------ evaluation counts
// Every limit of include/mvlpt_hip.h is checked here, before a launch (evaluate.hip).
int mvlpt_op_eval_count(const float* logits, int64_t ld, int B, int C, const void* labels, int label_kind, int64_t label_ld,
                        const int32_t* rows, int n_rows, const int32_t* task, const int32_t* lo, const int32_t* hi, int T,
                        const uint8_t* col_mask, uint8_t* col_seen, int64_t* n_true, int64_t* n_pred, int64_t* n_hit, int64_t* n_pred_r,
                        int64_t* n_hit_r, int64_t* cmat, mvlpt_stream_t stream) {
  if (!logits || !labels || !n_true || !n_pred || !n_hit) return fail(nullptr, MVLPT_ERR_ARG, "op_eval_count: null argument");
  if (B < 1 || C < 1 || ld < C) return fail(nullptr, MVLPT_ERR_ARG, "op_eval_count: B and C must be at least 1 and the row pitch at least C");
  if (label_kind != MVLPT_LABEL_INT64 && label_kind != MVLPT_LABEL_PROB_F32) return fail(nullptr, MVLPT_ERR_ARG, "op_eval_count: unknown label kind");
  if (label_kind == MVLPT_LABEL_PROB_F32 && label_ld < C) return fail(nullptr, MVLPT_ERR_ARG, "op_eval_count: the label pitch must be at least C");
  if (rows && n_rows < 0) return fail(nullptr, MVLPT_ERR_ARG, "op_eval_count: n_rows must not be negative");
  const bool ranged = task || lo || hi;
  if (ranged && (!task || !lo || !hi || T < 1 || !n_pred_r || !n_hit_r))
    return fail(nullptr, MVLPT_ERR_ARG, "op_eval_count: task ranges need task, lo, hi, T >= 1, n_pred_r and n_hit_r together");
  if (cmat && (int64_t)C * C > ((int64_t)1 << 31)) return fail(nullptr, MVLPT_ERR_ARG, "op_eval_count: the confusion matrix needs C * C <= 2^31");
  EvalCountArgs a;
  a.logits = logits; a.ld = ld; a.B = B; a.C = C;
  a.label_i = label_kind == MVLPT_LABEL_INT64 ? (const long long*)labels : nullptr;
  a.label_f = label_kind == MVLPT_LABEL_PROB_F32 ? (const float*)labels : nullptr;
  a.label_ld = label_ld;
  a.rows = rows; a.n = rows ? n_rows : B;
  a.task = ranged ? task : nullptr; a.lo = lo; a.hi = hi; a.T = T;
  a.col_mask = col_mask; a.col_seen = col_seen;
  a.n_true = n_true; a.n_pred = n_pred; a.n_hit = n_hit; a.n_pred_r = n_pred_r; a.n_hit_r = n_hit_r; a.cmat = cmat;
  OPCHK(launch_eval_count(a, (hipStream_t)stream));
  return 0;
}
static int eval_rank_check(const char* who, int N, int C) {
  if (N < 1 || C < 1) return fail(nullptr, MVLPT_ERR_ARG, std::string(who) + ": N and C must be at least 1");
  if (N > MVLPT_EVAL_MAX_ROWS) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, std::string(who) + ": N exceeds MVLPT_EVAL_MAX_ROWS");
  return 0;
}
int mvlpt_eval_workspace_bytes(int N, int C, mvlpt_stream_t stream, int64_t* out) {
  if (!out) return fail(nullptr, MVLPT_ERR_ARG, "eval_workspace_bytes: null argument");
  if (int rc = eval_rank_check("eval_workspace_bytes", N, C)) return rc;
  *out = (int64_t)eval_rank_plan(N, C, stream_cus((hipStream_t)stream)).ws_bytes;
  return 0;
}
int mvlpt_op_eval_rank_columns(const float* scores, int64_t ld, int N, int C, const void* targets, int target_kind, int64_t target_ld,
                               const int32_t* rows, int n_rows, const double* thresholds, int64_t* n_pos, int64_t* n_neg,
                               int64_t* twice_u, double* interp, int32_t* flags, void* workspace, int64_t workspace_bytes,
                               mvlpt_stream_t stream) {
  if (!scores || !targets || !thresholds || !n_pos || !n_neg || !twice_u || !interp || !flags) return fail(nullptr, MVLPT_ERR_ARG, "op_eval_rank_columns: null argument");
  if (int rc = eval_rank_check("op_eval_rank_columns", N, C)) return rc;
  if (ld < C) return fail(nullptr, MVLPT_ERR_ARG, "op_eval_rank_columns: the row pitch must be at least C");
  if (target_kind != MVLPT_LABEL_INT64 && target_kind != MVLPT_LABEL_PROB_F32) return fail(nullptr, MVLPT_ERR_ARG, "op_eval_rank_columns: unknown target kind");
  if (target_kind == MVLPT_LABEL_PROB_F32 && target_ld < C) return fail(nullptr, MVLPT_ERR_ARG, "op_eval_rank_columns: the target pitch must be at least C");
  if (rows && (n_rows < 0 || n_rows > N)) return fail(nullptr, MVLPT_ERR_ARG, "op_eval_rank_columns: n_rows must lie in [0, N]");
  const int n = rows ? n_rows : N;
  const EvalRankPlan p = eval_rank_plan(n, C, stream_cus((hipStream_t)stream));
  if (p.ws_bytes && (!workspace || workspace_bytes < 0 || (uint64_t)workspace_bytes < p.ws_bytes || ((uintptr_t)workspace & 7) != 0))
    return fail(nullptr, MVLPT_ERR_ARG, "op_eval_rank_columns: the workspace is smaller than mvlpt_eval_workspace_bytes (" +
                                            std::to_string(p.ws_bytes) + " bytes), or not 8-byte aligned");
  OPCHK(launch_eval_rank_columns(scores, ld, N, C, target_kind == MVLPT_LABEL_INT64 ? (const long long*)targets : nullptr,
                                 target_kind == MVLPT_LABEL_PROB_F32 ? (const float*)targets : nullptr, target_ld, rows, n, thresholds,
                                 (long long*)n_pos, (long long*)n_neg, (long long*)twice_u, interp, flags, workspace, p,
                                 (hipStream_t)stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------ softmax regression (linear probe)
// Every limit of include/mvlpt_hip.h is checked here, before a launch: the kernels (softmax_reg.hip) trust their arguments.
static int softmax_reg_check(const char* who, int N, int D, int K) {
  const std::string w = std::string(who) + ": ";
  if (N < 1) return fail(nullptr, MVLPT_ERR_ARG, w + "N must be at least 1");
  if (K < 2) return fail(nullptr, MVLPT_ERR_ARG, w + "K must be at least 2");
  if (D < 4 || D % 4) return fail(nullptr, MVLPT_ERR_ARG, w + "D must be a multiple of 4, at least 4");
  if ((int64_t)K * ((int64_t)D + 1) >= ((int64_t)1 << 31)) return fail(nullptr, MVLPT_ERR_ARG, w + "K * (D + 1) must stay below 2^31");
  return 0;
}
static int softmax_reg_ws_check(const char* who, const void* ws, size_t have, size_t need) {
  if (have < need || ((uintptr_t)ws & 15) != 0)
    return fail(nullptr, MVLPT_ERR_ARG, std::string(who) + ": the workspace is smaller than needed (" + std::to_string(need) + " bytes), or not 16-byte aligned");
  return 0;
}
int mvlpt_softmax_reg_workspace_bytes(int N, int D, int K, size_t* bytes) {
  if (!bytes) return fail(nullptr, MVLPT_ERR_ARG, "softmax_reg_workspace_bytes: null argument");
  if (int rc = softmax_reg_check("softmax_reg_workspace_bytes", N, D, K)) return rc;
  *bytes = softmax_reg_plan(N, D, K).ws_bytes;
  return 0;
}
int mvlpt_op_softmax_reg_eval(const float* X, const int32_t* y, const float* theta, const float* dir, int N, int D, int K, double l2,
                              float* grad, double* stats, void* ws, size_t ws_bytes, mvlpt_stream_t stream) {
  if (!X || !y || !theta || !grad || !stats || !ws) return fail(nullptr, MVLPT_ERR_ARG, "op_softmax_reg_eval: null argument");
  if (int rc = softmax_reg_check("op_softmax_reg_eval", N, D, K)) return rc;
  if (!(l2 >= 0.0)) return fail(nullptr, MVLPT_ERR_ARG, "op_softmax_reg_eval: l2 must be a number >= 0");
  if ((((uintptr_t)X | (uintptr_t)theta) & 15) != 0 || ((uintptr_t)stats & 7) != 0)
    return fail(nullptr, MVLPT_ERR_ARG, "op_softmax_reg_eval: X and theta must be 16-byte aligned, stats 8-byte aligned");
  const SoftmaxRegPlan p = softmax_reg_plan(N, D, K);
  if (int rc = softmax_reg_ws_check("op_softmax_reg_eval", ws, ws_bytes, p.ws_bytes)) return rc;
  OPCHK(launch_softmax_reg_eval(X, y, theta, dir, N, D, K, l2, grad, stats, ws, p, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_softmax_reg_predict(const float* X, const float* theta, int N, int D, int K, int32_t* pred, float* margin, void* ws,
                                 size_t ws_bytes, mvlpt_stream_t stream) {
  if (!X || !theta || !pred || !ws) return fail(nullptr, MVLPT_ERR_ARG, "op_softmax_reg_predict: null argument");
  if (int rc = softmax_reg_check("op_softmax_reg_predict", N, D, K)) return rc;
  if ((((uintptr_t)X | (uintptr_t)theta) & 15) != 0)
    return fail(nullptr, MVLPT_ERR_ARG, "op_softmax_reg_predict: X and theta must be 16-byte aligned");
  const SoftmaxRegPlan p = softmax_reg_plan(N, D, K);
  if (int rc = softmax_reg_ws_check("op_softmax_reg_predict", ws, ws_bytes, p.predict_bytes)) return rc;
  OPCHK(launch_softmax_reg_predict(X, theta, N, D, K, pred, margin, ws, p, (hipStream_t)stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------ Tip-Adapter head
// Every limit of include/mvlpt_hip.h is checked here, before a launch: the kernels (tip.hip) trust their arguments.
static int tip_check(const char* who, int N, int NK, int C, int D, int nb, int na, int mode) {
  const std::string w = std::string(who) + ": ";
  if (mode != MVLPT_TIP_LOGITS && mode != MVLPT_TIP_TRAIN && mode != MVLPT_TIP_SEARCH) return fail(nullptr, MVLPT_ERR_ARG, w + "unknown mode");
  if (N < 1 || NK < 1 || N > MVLPT_TIP_MAX_ROWS || NK > MVLPT_TIP_MAX_ROWS)
    return fail(nullptr, MVLPT_ERR_ARG, w + "N and NK must lie in [1, MVLPT_TIP_MAX_ROWS]");
  if (C < 1 || C > MVLPT_TIP_MAX_CLASSES) return fail(nullptr, MVLPT_ERR_ARG, w + "C must lie in [1, MVLPT_TIP_MAX_CLASSES]");
  if (D < 4 || D % 4) return fail(nullptr, MVLPT_ERR_ARG, w + "D must be a multiple of 4, at least 4");
  if ((int64_t)N * C >= ((int64_t)1 << 31)) return fail(nullptr, MVLPT_ERR_ARG, w + "N * C must stay below 2^31 (chunk the rows)");
  if (mode == MVLPT_TIP_SEARCH) {
    if (nb < 1 || nb > MVLPT_TIP_MAX_NB) return fail(nullptr, MVLPT_ERR_ARG, w + "nb must lie in [1, MVLPT_TIP_MAX_NB]");
    if (na < 1 || na > MVLPT_TIP_MAX_NA) return fail(nullptr, MVLPT_ERR_ARG, w + "na must lie in [1, MVLPT_TIP_MAX_NA]");
  }
  return 0;
}
static int tip_ws_check(const char* who, const void* ws, int64_t have, size_t need) {
  if (!ws || have < 0 || (uint64_t)have < need || ((uintptr_t)ws & 15) != 0)
    return fail(nullptr, MVLPT_ERR_ARG, std::string(who) + ": the workspace is smaller than mvlpt_tip_workspace_bytes (" +
                                            std::to_string(need) + " bytes), or not 16-byte aligned");
  return 0;
}
int mvlpt_tip_workspace_bytes(int N, int NK, int C, int D, int nb, int na, int mode, int64_t* bytes) {
  if (!bytes) return fail(nullptr, MVLPT_ERR_ARG, "tip_workspace_bytes: null argument");
  if (int rc = tip_check("tip_workspace_bytes", N, NK, C, D, nb, na, mode)) return rc;
  *bytes = (int64_t)tip_plan(N, NK, C, D, nb, na, mode).ws_bytes;
  return 0;
}
int mvlpt_op_tip_logits(const float* F, const float* K, const int32_t* key_ptr, const float* W, float s, float alpha, float beta, int N,
                        int NK, int C, int D, float* logits, mvlpt_stream_t stream) {
  if (!F || !K || !key_ptr || !W || !logits) return fail(nullptr, MVLPT_ERR_ARG, "op_tip_logits: null argument");
  if (int rc = tip_check("op_tip_logits", N, NK, C, D, 0, 0, MVLPT_TIP_LOGITS)) return rc;
  if ((((uintptr_t)F | (uintptr_t)K | (uintptr_t)W) & 15) != 0) return fail(nullptr, MVLPT_ERR_ARG, "op_tip_logits: F, K and W must be 16-byte aligned");
  OPCHK(launch_tip_logits(F, K, key_ptr, W, s, alpha, beta, N, NK, C, D, logits, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_tip_train_fwd(const float* F, const int32_t* y, const float* K, const int32_t* key_ptr, const float* W, float s, float alpha,
                           float beta, int N, int NK, int C, int D, float* loss, int32_t* correct, float* logits, void* workspace,
                           int64_t workspace_bytes, mvlpt_stream_t stream) {
  if (!F || !y || !K || !key_ptr || !W || !loss || !correct) return fail(nullptr, MVLPT_ERR_ARG, "op_tip_train_fwd: null argument");
  if (int rc = tip_check("op_tip_train_fwd", N, NK, C, D, 0, 0, MVLPT_TIP_TRAIN)) return rc;
  if ((((uintptr_t)F | (uintptr_t)K | (uintptr_t)W) & 15) != 0) return fail(nullptr, MVLPT_ERR_ARG, "op_tip_train_fwd: F, K and W must be 16-byte aligned");
  const TipPlan p = tip_plan(N, NK, C, D, 0, 0, MVLPT_TIP_TRAIN);
  if (int rc = tip_ws_check("op_tip_train_fwd", workspace, workspace_bytes, p.ws_bytes)) return rc;
  OPCHK(launch_tip_train_fwd(F, y, K, key_ptr, W, s, alpha, beta, N, NK, C, D, loss, correct, logits, workspace, p, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_tip_train_bwd(const float* F, float alpha, float beta, int N, int NK, int C, int D, float* dK, void* workspace,
                           int64_t workspace_bytes, mvlpt_stream_t stream) {
  if (!F || !dK) return fail(nullptr, MVLPT_ERR_ARG, "op_tip_train_bwd: null argument");
  if (int rc = tip_check("op_tip_train_bwd", N, NK, C, D, 0, 0, MVLPT_TIP_TRAIN)) return rc;
  if ((((uintptr_t)F | (uintptr_t)dK) & 15) != 0) return fail(nullptr, MVLPT_ERR_ARG, "op_tip_train_bwd: F and dK must be 16-byte aligned");
  const TipPlan p = tip_plan(N, NK, C, D, 0, 0, MVLPT_TIP_TRAIN);
  if (int rc = tip_ws_check("op_tip_train_bwd", workspace, workspace_bytes, p.ws_bytes)) return rc;
  OPCHK(launch_tip_train_bwd(F, alpha, beta, N, NK, C, D, dK, workspace, p, (hipStream_t)stream));
  return 0;
}
int mvlpt_op_tip_search(const float* F, const int32_t* y, const float* K, const int32_t* key_ptr, const float* W, float s,
                        const float* betas, const float* alphas, int N, int NK, int C, int D, int nb, int na, int32_t* counts,
                        void* workspace, int64_t workspace_bytes, mvlpt_stream_t stream) {
  if (!F || !y || !K || !key_ptr || !W || !betas || !alphas || !counts) return fail(nullptr, MVLPT_ERR_ARG, "op_tip_search: null argument");
  if (int rc = tip_check("op_tip_search", N, NK, C, D, nb, na, MVLPT_TIP_SEARCH)) return rc;
  if ((((uintptr_t)F | (uintptr_t)K | (uintptr_t)W) & 15) != 0) return fail(nullptr, MVLPT_ERR_ARG, "op_tip_search: F, K and W must be 16-byte aligned");
  const TipPlan p = tip_plan(N, NK, C, D, nb, na, MVLPT_TIP_SEARCH);
  if (int rc = tip_ws_check("op_tip_search", workspace, workspace_bytes, p.ws_bytes)) return rc;
  OPCHK(launch_tip_search(F, y, K, key_ptr, W, s, betas, alphas, N, NK, C, D, nb, na, counts, workspace, p, (hipStream_t)stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------ input pipeline
// One pass over a batch's descriptors for the entry `who`: every box inside its image, every image inside src, and the output window
// inside the resized image, or, under fill_outside, merely near enough to it for 32-bit arithmetic; `why` is the entry's wording of
// that.  aug (may be null): the augmentation of image b is checked right behind its descriptor.  Returns the tallest crop and the
// widest filter footprint of the batch.
static int pp_check(Engine* E, const char* who, const char* why, const MvlptImageDesc* descs, const MvlptAugmentDesc* aug, int B,
                    int64_t src_bytes, int out_h, int out_w, int fill_outside, int* max_crop_h, int* ks_max) {
  const int64_t far = (int64_t)1 << 30;
  for (int b = 0; b < B; ++b) {
    const MvlptImageDesc& d = descs[b];
    bool ok = d.height > 0 && d.width > 0 && d.offset >= 0 && d.offset + (int64_t)d.height * d.width * 3 <= src_bytes &&
              d.crop_top >= 0 && d.crop_left >= 0 && d.crop_height > 0 && d.crop_width > 0 &&
              d.crop_top + d.crop_height <= d.height && d.crop_left + d.crop_width <= d.width && d.resize_height > 0 &&
              d.resize_width > 0 && (d.flip == 0 || d.flip == 1);
    if (fill_outside) ok = ok && d.out_top >= -far && d.out_top <= far && d.out_left >= -far && d.out_left <= far;
    else ok = ok && d.out_top >= 0 && d.out_left >= 0 && (int64_t)d.out_top + out_h <= d.resize_height && (int64_t)d.out_left + out_w <= d.resize_width;
    if (!ok) return fail(E, MVLPT_ERR_ARG, std::string(who) + ": descriptor " + std::to_string(b) + " is inconsistent (" + why + ")");
    *max_crop_h = std::max(*max_crop_h, (int)d.crop_height);
    const double sh = std::max(1.0, (double)d.crop_height / d.resize_height), sw = std::max(1.0, (double)d.crop_width / d.resize_width);
    *ks_max = std::max(*ks_max, std::max((int)std::ceil(2.0 * sh), (int)std::ceil(2.0 * sw)) * 2 + 1);
    if (!aug) continue;
    const MvlptAugmentDesc& a = aug[b];
    ok = a.n_ops >= 0 && a.n_ops <= PP_AUG_MAX_OPS && (a.grayscale == 0 || a.grayscale == 1) && a.n_holes >= 0 && a.n_holes <= PP_AUG_MAX_HOLES;
    unsigned seen = 0;
    for (int k = 0; ok && k < a.n_ops; ++k) {
      const int op = a.ops[k];
      ok = op >= 0 && op <= PP_OP_HUE && !(seen >> op & 1u);
      if (!ok) break;
      seen |= 1u << op;
      if (op == PP_OP_HUE) ok = a.hue_shift >= 0 && a.hue_shift <= 255;
      else ok = std::isfinite(a.factor[op]) && a.factor[op] >= 0.0f;
    }
    for (int k = 0; ok && k < a.n_holes; ++k) {
      const int32_t* r = a.hole[k];
      ok = r[0] >= 0 && r[1] >= 0 && r[2] >= 1 && r[3] >= 1 && (int64_t)r[0] + r[2] <= out_h && (int64_t)r[1] + r[3] <= out_w;
    }
    if (!ok) return fail(E, MVLPT_ERR_ARG, std::string(who) + ": augmentation " + std::to_string(b) + " is malformed (operation count / id / repeat, factor not finite or negative, hue_shift, grayscale, or a hole outside the window)");
  }
  return 0;
}
// where the parts of pp_ws lie: [image descs | augmentations (with_aug) | resampling tables | row-pass output | windows (with_win)]
struct PpLayout {
  size_t table_stride = 0, tmp_stride = 0;      // int32 per (image, pass); bytes per image
  size_t augs = 0, tables = 0, tmp = 0, win = 0, total = 0;
  PpLayout(int B, int max_crop_h, int ks_max, int out_h, int out_w, bool with_aug, bool with_win) {
    table_stride = (size_t)(2 + ks_max) * std::max(out_h, out_w);
    tmp_stride = align256((size_t)max_crop_h * out_w * 3);
    augs = align256(sizeof(PpDesc) * (size_t)B);
    tables = augs + (with_aug ? align256(sizeof(PpAug) * (size_t)B) : 0);
    tmp = tables + align256(table_stride * 4 * 2 * (size_t)B);
    win = tmp + align256(tmp_stride * (size_t)B);
    total = win + (with_win ? (size_t)B * out_h * out_w * 3 : 0);
  }
};

int mvlpt_preprocess(void* h, const uint8_t* src, int64_t src_bytes, const MvlptImageDesc* descs, int B, int out_h, int out_w,
                     const float* mean, const float* stdv, void* out, int out_dtype, uint8_t* out_u8, mvlpt_stream_t stream) {
  static_assert(sizeof(MvlptImageDesc) == sizeof(PpDesc), "descriptor layouts must match");
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  if (!src || !descs || B <= 0 || out_h <= 0 || out_w <= 0 || !mean || !stdv || (!out && !out_u8))
    return fail(E, MVLPT_ERR_ARG, "preprocess: null pointer or empty batch / output");
  if (out && out_dtype != DT_F32 && out_dtype != DT_F16 && out_dtype != DT_BF16) return fail(E, MVLPT_ERR_ARG, "preprocess: bad out_dtype");
  int max_crop_h = 0, ks_max = 1;
  if (int rc = pp_check(E, "preprocess", "box / window outside the image, or image outside src", descs, nullptr, B, src_bytes, out_h, out_w, 0,
                        &max_crop_h, &ks_max))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  const PpLayout lay(B, max_crop_h, ks_max, out_h, out_w, false, false);
  HIPCHK(E, E->pp_ws.reserve(lay.total));
  char* base = (char*)E->pp_ws.p;
  PpDesc* descs_dev = (PpDesc*)base;
  HIPCHK(E, hipMemcpyAsync(descs_dev, descs, sizeof(PpDesc) * (size_t)B, hipMemcpyHostToDevice, s));
  HIPCHK(E, launch_preprocess(src, descs_dev, B, max_crop_h, ks_max, out_h, out_w, (int32_t*)(base + lay.tables), lay.table_stride,
                              (uint8_t*)(base + lay.tmp), lay.tmp_stride, mean, stdv, out, out_dtype, out_u8, s));
  return 0;
}

int mvlpt_preprocess_aug(void* h, const uint8_t* src, int64_t src_bytes, const MvlptImageDesc* descs, const MvlptAugmentDesc* aug, int B,
                         int out_h, int out_w, int fill_outside, const float* mean, const float* stdv, void* out, int out_dtype,
                         uint8_t* out_u8, mvlpt_stream_t stream) {
  static_assert(sizeof(MvlptAugmentDesc) == sizeof(PpAug) && MVLPT_AUG_MAX_HOLES == PP_AUG_MAX_HOLES, "descriptor layouts must match");
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  if (B < 0 || (fill_outside != 0 && fill_outside != 1)) return fail(E, MVLPT_ERR_ARG, "preprocess_aug: negative batch, or fill_outside is not 0 or 1");
  if (B == 0) return 0;
  if (!aug && !fill_outside) return mvlpt_preprocess(h, src, src_bytes, descs, B, out_h, out_w, mean, stdv, out, out_dtype, out_u8, stream);
  if (!src || !descs || out_h <= 0 || out_w <= 0 || (int64_t)out_h * out_w > (1 << 29) || !mean || !stdv || (!out && !out_u8))
    return fail(E, MVLPT_ERR_ARG, "preprocess_aug: null pointer or empty / oversized output");
  if (out && out_dtype != DT_F32 && out_dtype != DT_F16 && out_dtype != DT_BF16) return fail(E, MVLPT_ERR_ARG, "preprocess_aug: bad out_dtype");
  int max_crop_h = 0, ks_max = 1;
  if (int rc = pp_check(E, "preprocess_aug", "box outside the image, image outside src, or window outside the resized image without fill_outside",
                        descs, aug, B, src_bytes, out_h, out_w, fill_outside, &max_crop_h, &ks_max))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  const PpLayout lay(B, max_crop_h, ks_max, out_h, out_w, true, !out_u8);            // the colour stage works in out_u8 when it is asked for
  HIPCHK(E, E->pp_ws.reserve(lay.total));
  char* base = (char*)E->pp_ws.p;
  PpDesc* descs_dev = (PpDesc*)base;
  PpAug* augs_dev = (PpAug*)(base + lay.augs);
  HIPCHK(E, hipMemcpyAsync(descs_dev, descs, sizeof(PpDesc) * (size_t)B, hipMemcpyHostToDevice, s));
  if (aug) HIPCHK(E, hipMemcpyAsync(augs_dev, aug, sizeof(PpAug) * (size_t)B, hipMemcpyHostToDevice, s));
  else HIPCHK(E, hipMemsetAsync(augs_dev, 0, sizeof(PpAug) * (size_t)B, s));
  HIPCHK(E, launch_preprocess_aug(src, descs_dev, augs_dev, B, max_crop_h, ks_max, out_h, out_w, (int32_t*)(base + lay.tables),
                                  lay.table_stride, (uint8_t*)(base + lay.tmp), lay.tmp_stride, out_u8 ? out_u8 : (uint8_t*)(base + lay.win),
                                  mean, stdv, out, out_dtype, s));
  return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ JPEG decode
namespace {
static_assert(sizeof(MvlptJpegInfo) == sizeof(jpeg::Info), "info layouts must match");
static_assert(MVLPT_JPEG_ROUTE_SIZE == jpeg::ROUTE_SIZE && MVLPT_JPEG_ST_BAD_SIZE == jpeg::ST_BAD_SIZE, "route / status codes must match");
constexpr int JPEG_MAX_BATCH = 16384;            // images and 3 x planes ride on grid.y

// where the parts of a decode's workspace lie: [image descs | plane descs | table sets | segment table] (uploaded as one block), then
// the coefficient blocks and the component planes
struct JpegLayout {
  size_t descs = 0, planes = 0, tables = 0, segs = 0, meta = 0, coefs = 0, pix = 0, total = 0;
  JpegLayout(size_t n_images, size_t n_segs, int64_t coef_blocks, int64_t plane_bytes) {
    descs = 0;
    planes = descs + align256(n_images * sizeof(jpeg::ImgDesc));
    tables = planes + align256(3 * n_images * sizeof(jpeg::PlaneDesc));
    segs = tables + align256(n_images * sizeof(jpeg::Tables));
    meta = segs + align256(n_segs * sizeof(jpeg::Seg));
    coefs = meta;
    pix = coefs + align256((size_t)coef_blocks * 128);
    total = pix + align256((size_t)plane_bytes);
  }
};
}  // namespace

extern "C" {

int mvlpt_jpeg_probe(const uint8_t* bytes, int64_t n, MvlptJpegInfo* info) {
  if (!bytes || !info || n < 0) return fail(nullptr, MVLPT_ERR_ARG, "jpeg_probe: null argument or negative size");
  jpeg::Parsed P;
  jpeg::parse(bytes, (size_t)n, &P);
  if (P.info.route != jpeg::ROUTE_DEVICE) P.info.n_segments = 0;
  memcpy(info, &P.info, sizeof(*info));
  return 0;
}

int mvlpt_jpeg_workspace_bytes(const MvlptJpegInfo* infos, int B, int64_t* bytes) {
  if (!bytes || B < 0 || (B > 0 && !infos)) return fail(nullptr, MVLPT_ERR_ARG, "jpeg_workspace_bytes: null argument or negative batch");
  size_t n_images = 0, n_segs = 0;
  int64_t blocks = 0, pix = 0;
  for (int b = 0; b < B; ++b) {
    if (infos[b].route != MVLPT_JPEG_ROUTE_DEVICE) continue;
    jpeg::Info f;
    memcpy(&f, &infos[b], sizeof(f));
    const bool ok = f.height > 0 && f.width > 0 && (int64_t)f.height * f.width <= jpeg::MAX_PIXELS && (f.components == 1 || f.components == 3) &&
                    f.h_samp >= 1 && f.h_samp <= 4 && f.v_samp >= 1 && f.v_samp <= 4 && f.n_segments >= 1;
    if (!ok) return fail(nullptr, MVLPT_ERR_ARG, "jpeg_workspace_bytes: info " + std::to_string(b) + " is not one mvlpt_jpeg_probe returns");
    const jpeg::Geom g = jpeg::geometry(f);
    ++n_images; n_segs += (size_t)f.n_segments; blocks += g.total_blocks; pix += g.total_plane_bytes;
  }
  *bytes = (int64_t)JpegLayout(n_images, n_segs, blocks, pix).total;
  return 0;
}

int mvlpt_jpeg_decode(void* h, const uint8_t* src_host, const uint8_t* src_dev, const int64_t* src_offsets, const int64_t* src_sizes, int B,
                      uint8_t* dst_dev, int64_t dst_bytes, const int64_t* dst_offsets, int32_t* status_dev, mvlpt_stream_t stream) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  if (B < 0 || B > JPEG_MAX_BATCH) return fail(E, MVLPT_ERR_ARG, "jpeg_decode: batch negative or above 16384");
  if (B == 0) return 0;
  if (!src_host || !src_dev || !src_offsets || !src_sizes || !dst_dev || !dst_offsets || !status_dev || dst_bytes < 0)
    return fail(E, MVLPT_ERR_ARG, "jpeg_decode: null argument");
  std::vector<jpeg::Parsed> parsed((size_t)B);
  size_t n_images = 0, n_segs = 0;
  int64_t blocks = 0, pix = 0;
  for (int b = 0; b < B; ++b) {
    if (src_offsets[b] < 0 || src_sizes[b] < 0) return fail(E, MVLPT_ERR_ARG, "jpeg_decode: negative source offset or size at " + std::to_string(b));
    jpeg::parse(src_host + src_offsets[b], (size_t)src_sizes[b], &parsed[b]);
    const jpeg::Info& f = parsed[b].info;
    if (f.route != jpeg::ROUTE_DEVICE) continue;
    if (dst_offsets[b] < 0 || dst_offsets[b] > dst_bytes || (int64_t)f.height * f.width * 3 > dst_bytes - dst_offsets[b])
      return fail(E, MVLPT_ERR_ARG, "jpeg_decode: image " + std::to_string(b) + " (" + std::to_string(f.height) + " x " + std::to_string(f.width) +
                                        ") does not fit dst_bytes at its offset");
    const jpeg::Geom g = jpeg::geometry(f);
    ++n_images; n_segs += parsed[b].segs.size(); blocks += g.total_blocks; pix += g.total_plane_bytes;
  }
  hipStream_t s = (hipStream_t)stream;
  E->jpeg_status_host.assign((size_t)B, -1);
  for (int b = 0; b < B; ++b) if (parsed[b].info.route == jpeg::ROUTE_DEVICE) E->jpeg_status_host[b] = 0;
  HIPCHK(E, hipMemcpyAsync(status_dev, E->jpeg_status_host.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
  if (n_images == 0) return 0;
  const JpegLayout lay(n_images, n_segs, blocks, pix);
  HIPCHK(E, E->jpeg_ws.reserve(lay.total));
  E->jpeg_meta_host.assign(lay.meta, 0);
  uint8_t* mh = E->jpeg_meta_host.data();
  jpeg::ImgDesc* descs = (jpeg::ImgDesc*)(mh + lay.descs);
  jpeg::PlaneDesc* planes = (jpeg::PlaneDesc*)(mh + lay.planes);
  jpeg::Tables* tables = (jpeg::Tables*)(mh + lay.tables);
  jpeg::Seg* segs = (jpeg::Seg*)(mh + lay.segs);
  int n_tables = 0, n_planes = 0, max_blocks = 0;
  size_t k = 0, seg_at = 0;
  int64_t coef_at = 0, pix_at = 0;
  long long max_groups = 0;
  for (int b = 0; b < B; ++b) {
    const jpeg::Parsed& P = parsed[b];
    if (P.info.route != jpeg::ROUTE_DEVICE) continue;
    if (n_tables == 0 || memcmp(&tables[n_tables - 1], &P.tables, sizeof(jpeg::Tables)) != 0) tables[n_tables++] = P.tables;   // shared with the previous image when equal
    const jpeg::ImgDesc d = jpeg::describe(P, src_offsets[b], dst_offsets[b], coef_at, pix_at, (int)seg_at, n_tables - 1, b);
    descs[k++] = d;
    for (int c = 0; c < d.ncomp; ++c) {
      jpeg::PlaneDesc& p = planes[n_planes++];
      p.coef_off = d.coef_off[c]; p.plane_off = d.plane_off[c];
      p.n_blocks = d.blocks_w[c] * (d.plane_h[c] / 8); p.blocks_w = d.blocks_w[c]; p.plane_w = d.plane_w[c];
      p.tables = d.tables; p.tq = d.tq[c]; p.reserved = 0;
      max_blocks = std::max(max_blocks, p.n_blocks);
    }
    for (const jpeg::Seg& sg : P.segs) segs[seg_at++] = sg;
    const jpeg::Geom g = jpeg::geometry(P.info);
    coef_at += g.total_blocks; pix_at += g.total_plane_bytes;
    max_groups = std::max(max_groups, (long long)((d.width + 3) >> 2) * d.height);
  }
  char* base = (char*)E->jpeg_ws.p;
  int16_t* coefs_dev = (int16_t*)(base + lay.coefs);
  uint8_t* pix_dev = (uint8_t*)(base + lay.pix);
  HIPCHK(E, hipMemcpyAsync(base, mh, lay.meta, hipMemcpyHostToDevice, s));
  HIPCHK(E, hipMemsetAsync(coefs_dev, 0, (size_t)blocks * 128, s));
  HIPCHK(E, launch_jpeg_entropy(src_dev, (const jpeg::ImgDesc*)(base + lay.descs), (const jpeg::Tables*)(base + lay.tables),
                                (const jpeg::Seg*)(base + lay.segs), (int)n_images, coefs_dev, status_dev, s));
  HIPCHK(E, launch_jpeg_idct((const jpeg::PlaneDesc*)(base + lay.planes), n_planes, max_blocks, (const jpeg::Tables*)(base + lay.tables), coefs_dev,
                             pix_dev, s));
  HIPCHK(E, launch_jpeg_colour((const jpeg::ImgDesc*)(base + lay.descs), (int)n_images, max_groups, pix_dev, dst_dev, s));
  return 0;
}

int mvlpt_op_jpeg_entropy(const uint8_t* file_host, int64_t n, const uint8_t* file_dev, void* ws, int64_t ws_bytes, int16_t* coefs,
                          int64_t coef_blocks, int32_t* status_dev, mvlpt_stream_t stream) {
  if (!file_host || !file_dev || !ws || !coefs || !status_dev || n < 0) return fail(nullptr, MVLPT_ERR_ARG, "op_jpeg_entropy: null argument");
  static thread_local jpeg::Parsed P;
  static thread_local std::vector<uint8_t> host;
  jpeg::parse(file_host, (size_t)n, &P);
  if (P.info.route != jpeg::ROUTE_DEVICE) return fail(nullptr, MVLPT_ERR_UNSUPPORTED, "op_jpeg_entropy: route " + std::to_string(P.info.route) + ", not a file the device decodes");
  const jpeg::Geom g = jpeg::geometry(P.info);
  const size_t need = 4096 + 8 * P.segs.size();
  if (coef_blocks != g.total_blocks || ws_bytes < (int64_t)need || ((uintptr_t)ws & 15))
    return fail(nullptr, MVLPT_ERR_ARG, "op_jpeg_entropy: coef_blocks must be " + std::to_string(g.total_blocks) + " and ws hold " + std::to_string(need) + " bytes, 16-byte aligned");
  static_assert(sizeof(jpeg::ImgDesc) <= 512 && sizeof(jpeg::Tables) <= 3584, "the op's scratch layout");
  host.assign(need, 0);
  const jpeg::ImgDesc d = jpeg::describe(P, 0, 0, 0, 0, 0, 0, 0);
  memcpy(host.data(), &d, sizeof(d));
  memcpy(host.data() + 512, &P.tables, sizeof(P.tables));
  memcpy(host.data() + 4096, P.segs.data(), 8 * P.segs.size());
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  OPCHK(hipMemcpyAsync(base, host.data(), need, hipMemcpyHostToDevice, s));
  OPCHK(hipMemsetAsync(coefs, 0, (size_t)coef_blocks * 128, s));
  OPCHK(launch_jpeg_entropy(file_dev, (const jpeg::ImgDesc*)base, (const jpeg::Tables*)(base + 512), (const jpeg::Seg*)(base + 4096), 1, coefs,
                            status_dev, s));
  return 0;
}

int mvlpt_op_jpeg_idct(const int16_t* coefs, const uint8_t* quant, int n_blocks, int blocks_w, uint8_t* plane, mvlpt_stream_t stream) {
  if (!coefs || !quant || !plane || n_blocks <= 0 || blocks_w <= 0 || n_blocks % blocks_w || blocks_w > (1 << 20) || ((uintptr_t)plane & 7))
    return fail(nullptr, MVLPT_ERR_ARG, "op_jpeg_idct: null / misaligned pointer, or n_blocks is not a positive multiple of blocks_w");
  jpeg::PlaneDesc p = {};
  p.n_blocks = n_blocks; p.blocks_w = blocks_w; p.plane_w = blocks_w * 8;
  OPCHK(launch_jpeg_idct_one(p, quant, coefs, plane, (hipStream_t)stream));
  return 0;
}

int mvlpt_op_jpeg_colour(const uint8_t* planes, const int64_t* plane_off, const int32_t* plane_w, int components, int hs, int vs, int height,
                         int width, uint8_t* dst, mvlpt_stream_t stream) {
  const bool samp_ok = (hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2);
  if (!planes || !plane_off || !plane_w || !dst || (components != 1 && components != 3) || !samp_ok || height <= 0 || width <= 0 ||
      (int64_t)height * width > jpeg::MAX_PIXELS) return fail(nullptr, MVLPT_ERR_ARG, "op_jpeg_colour: null / invalid argument");
  jpeg::ImgDesc d;
  memset(&d, 0, sizeof(d));
  d.width = width; d.height = height; d.ncomp = components; d.hs = components == 1 ? 1 : hs; d.vs = components == 1 ? 1 : vs;
  for (int c = 0; c < components; ++c) {
    const int need_w = c == 0 ? width : (width + d.hs - 1) / d.hs;
    if (plane_off[c] < 0 || plane_w[c] < need_w) return fail(nullptr, MVLPT_ERR_ARG, "op_jpeg_colour: a plane is narrower than its component");
    d.plane_off[c] = plane_off[c]; d.plane_w[c] = plane_w[c];
  }
  OPCHK(launch_jpeg_colour_one(d, planes, dst, (hipStream_t)stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------ profiling
int mvlpt_profile_begin(void* h, int all_kernels) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  E->prof.clear(); E->ev_used = 0; E->prof_on = true; E->prof_all = all_kernels != 0;
  return 0;
}
int mvlpt_profile_pause(void* h, int paused) {
  Engine* E = (Engine*)h;
  if (!E) return MVLPT_ERR_ARG;
  E->prof_on = !paused;
  return 0;
}
int mvlpt_profile_end(void* h, MvlptKernelStat* stats, int max_stats) {
  Engine* E = (Engine*)h;
  if (!E || !stats || max_stats <= 0) return MVLPT_ERR_ARG;
  E->prof_on = false;
  MvlptKernelStat acc[PC_COUNT];
  for (int i = 0; i < PC_COUNT; ++i) { memset(&acc[i], 0, sizeof(acc[i])); snprintf(acc[i].name, sizeof(acc[i].name), "%s", kProfNames[i]); }
  // ... and the GEMM launches once more per problem (M, N, K, epilogue, operand format, folded consumer): name "g<M>x<N>x<K> e<epi> s<split> f<fold>"
  std::map<std::array<int, 6>, MvlptKernelStat> shapes;
  std::vector<std::pair<float, float>> iv[PC_COUNT];     // [start, end] in ms relative to the first recorded event
  hipEvent_t ref = E->prof.empty() ? nullptr : E->prof.front().a;
  for (const ProfRec& r : E->prof) {
    if (hipEventSynchronize(r.b) != hipSuccess) continue;
    float ms = 0.f, t0 = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
    acc[r.cls].launches += 1; acc[r.cls].ms += ms; acc[r.cls].flops += r.flops; acc[r.cls].bytes += r.bytes;
    acc[r.cls].flops_executed += r.flops_exec;
    if (r.cls == PC_GEMM && r.M > 0) {
      MvlptKernelStat& q = shapes[{r.M, r.N, r.K, r.epi, r.split, r.fold}];
      if (!q.launches) { memset(&q, 0, sizeof(q)); snprintf(q.name, sizeof(q.name), "g%dx%dx%d e%d s%d f%d", r.M, r.N, r.K, r.epi, r.split, r.fold); }
      q.launches += 1; q.ms += ms; q.busy_ms += ms; q.flops += r.flops; q.bytes += r.bytes; q.flops_executed += r.flops_exec;
    }
    if (r.a == ref || hipEventElapsedTime(&t0, ref, r.a) == hipSuccess) iv[r.cls].push_back({t0, t0 + ms});
  }
  for (int c = 0; c < PC_COUNT; ++c) {                    // union of the intervals per class
    std::sort(iv[c].begin(), iv[c].end());
    double busy = 0.0; float cs = 0.f, ce = -1.f;
    for (auto& p : iv[c]) {
      if (ce < 0.f) { cs = p.first; ce = p.second; }
      else if (p.first > ce) { busy += ce - cs; cs = p.first; ce = p.second; }
      else if (p.second > ce) ce = p.second;
    }
    if (ce >= 0.f) busy += ce - cs;
    acc[c].busy_ms = busy;
  }
  int n = 0;
  for (int i = 0; i < PC_COUNT && n < max_stats; ++i) if (acc[i].launches) stats[n++] = acc[i];
  std::vector<MvlptKernelStat> by_time;
  for (auto& kv : shapes) by_time.push_back(kv.second);
  std::sort(by_time.begin(), by_time.end(), [](const MvlptKernelStat& x, const MvlptKernelStat& y) { return x.ms > y.ms; });
  for (size_t i = 0; i < by_time.size() && n < max_stats; ++i) stats[n++] = by_time[i];
  E->prof.clear(); E->ev_used = 0;
  return n;
}

}  // extern "C"
