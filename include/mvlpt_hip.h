/* libmvlpt_hip.so — C ABI of the MI355X-native prompted-CLIP hot path.
 *
 * Drop-in boundary for the reference's `CustomCLIP.forward` + loss/backward as driven by
 * `MVLPT.forward_backward` (reference: trainers/mvlpt.py:540-583 and :910-932).  The reference has no FFI
 * (it is pure Python on PyTorch ops), so each entry point below names the Python call site it replaces;
 * `INTEGRATION.md` shows the ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain C, raw DEVICE pointers + sizes, no torch types.  The caller (PyTorch-ROCm host code) owns every
 *     tensor buffer it passes; the library owns only its handle (packed frozen weights, saved activations,
 *     workspace).
 *   - every call only ENQUEUES work on `stream` (a hipStream_t): no hidden synchronisation, except that the
 *     first call at a new, larger problem size grows the workspace (hipMalloc).
 *   - return 0 on success, <0 on error; `mvlpt_last_error()` gives the message.  One handle per process per
 *     GPU, not thread-safe (the reference drives the device from a single Python thread).
 *   - prompt tensors and features cross the boundary as fp32; the towers compute in `compute_dtype`
 *     (fp16 or bf16 MFMA inputs, fp32 accumulation, fp32 residual stream, fp32 LayerNorm/softmax/CE).
 *   - token / class / task indexing is integer and exact.
 */
#ifndef MVLPT_HIP_H
#define MVLPT_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* mvlpt_stream_t; /* hipStream_t */

enum { MVLPT_DT_F32 = 0, MVLPT_DT_F16 = 1, MVLPT_DT_BF16 = 2 };
enum { MVLPT_LABEL_INT64 = 0, MVLPT_LABEL_PROB_F32 = 1 };
enum { MVLPT_ERR_ARG = -1, MVLPT_ERR_HIP = -2, MVLPT_ERR_STATE = -3, MVLPT_ERR_UNSUPPORTED = -4 };

/* Architecture of the frozen CLIP (same quantities clip.model.build_model infers, clip/model.py:395-418). */
typedef struct MvlptArch {
  int image_resolution, patch_size, vision_width, vision_layers, vision_heads;
  int context_length, text_width, text_layers, text_heads;
  int embed_dim;
  int compute_dtype; /* MVLPT_DT_F16 (reference default PREC, train.py:131) or MVLPT_DT_BF16 */
} MvlptArch;

/* Precision mode of the towers (reference knob: TRAINER.MVLPT.PREC, trainers/mvlpt.py:835-836, 848-850).
 * All modes: 16-bit MFMA operands, fp32 accumulation, fp32 residual stream / LayerNorm / softmax / cross-entropy.
 *   MVLPT_PREC_FAST       single 16-bit operands everywhere (prompt gradients within ~4e-3 of the fp32 CPU path)
 *   MVLPT_PREC_SPLIT_GRAD default: a tower whose forward is saved for a backward runs with SPLIT operands — every GEMM A
 *                         operand is hi = round16(x) plus its rounding residual as one e5m2 byte (the "mixed pair" below: the
 *                         residual term runs on the fp8 MFMA against an e4m3 copy of the frozen weight: e5m2 keeps 2 mantissa bits
 *                         of a residual that is <= 2^-11 |x| (fp16) / 2^-8 |x| (bf16), e4m3 3 bits of the weight, so an operand is
 *                         carried to ~2^-14 (fp16) / ~2^-11 (bf16) of its value — the per-element bounds tests/test_hip_mixed_pair.py
 *                         asserts; a K = 768 product lands at ~1e-5 relative against 2e-4 with single operands),
 *                         the attention core takes 16-bit hi+lo pairs with three-term products — so prompt gradients match the
 *                         fp32 CPU path to 1e-3; forward-only towers (e.g. the image tower under CoOp, inference) stay fast.
 *                         Environment MVLPT_SPLIT_LO8=0 selects 16-bit hi+lo pairs for the GEMMs as well (twice the matrix time)
 *   MVLPT_PREC_SPLIT_ALL  split operands in every tower, 16-bit hi+lo pairs (~22 bits) everywhere (PREC = "fp32") */
enum { MVLPT_PREC_FAST = 0, MVLPT_PREC_SPLIT_GRAD = 1, MVLPT_PREC_SPLIT_ALL = 2 };

/* A handle for a ViT image tower and the text tower.  Widths are multiples of 128 and embed_dim of 64.  The text tower's heads are 64
 * wide (text_width == text_heads * 64).  The image tower's head width vision_width / vision_heads is 64 (CLIP's own ViTs: heads =
 * width // 64) or one of 80, 96, 112, 128 (the ViT-H/14 family: width 1280 = 16 heads of 80); any other head width returns
 * MVLPT_ERR_UNSUPPORTED.  An image tower with heads wider than 64 is frozen, prompt-free and forward-only on single 16-bit operands
 * (CoOp, CoCoOp, zero-shot, feature extraction): mvlpt_image_fwd with n_vpt == 0 and save_for_bwd == 0 and mvlpt_image_fwd_begin /
 * _resume / _abandon run, at any token count; visual prompts, save_for_bwd != 0, mvlpt_image_bwd, mvlpt_set_vpt_dropout and an image
 * forward under MVLPT_PREC_SPLIT_ALL (whose forward-only towers run on pairs) return MVLPT_ERR_UNSUPPORTED with a message naming the
 * cause, without touching the device, and leave the handle usable. */
int mvlpt_create(const MvlptArch* arch, void** handle);
/* A handle whose image tower is CLIP's ModifiedResNet (clip/model.py:94-150: RN50, RN101; three-conv stem, four stages of Bottleneck
 * blocks of `layers[i]` blocks and width * {1,2,4,8} planes, AttentionPool2d with `heads` heads of 64 over 32 * width channels).
 * `arch` carries the text tower, embed_dim and compute_dtype; its ViT vision fields (image_resolution, patch_size, vision_width,
 * vision_layers, vision_heads) must be 0.  image_resolution % 32 == 0, width % 4 == 0, heads * 64 == 32 * width,
 * output_dim == embed_dim (MVLPT_ERR_ARG otherwise); compute_dtype must be MVLPT_DT_F16 (bf16: MVLPT_ERR_UNSUPPORTED).
 * The tower is frozen and forward-only, as every route of the reference that reaches it (trainers/coop.py:220, cocoop.py:169,
 * zsclip.py:56, lpclip/feat_extractor.py:155; trainers/mvlpt.py:48 cannot prompt a ResNet): NHWC fp16 activations, implicit-GEMM
 * convolutions on the fp16 MFMA with fp32 accumulation, BatchNorm (running statistics) as an fp32 scale / shift in the epilogue.
 * On such a handle
 *   - mvlpt_load_frozen takes the reference's keys visual.conv{1,2,3}.weight, visual.bn{1,2,3}.*, visual.layer{1..4}.{i}.conv{1,2,3}.weight,
 *     .bn{1,2,3}.*, .downsample.0.weight, .downsample.1.*, visual.attnpool.positional_embedding, visual.attnpool.{q,k,v,c}_proj.*;
 *   - mvlpt_image_fwd(handle, image, dtype, NULL, NULL, 0, 0, B, feat_out, 0, stream) runs the tower, enqueue-only;
 *   - visual prompts, save_for_bwd != 0, mvlpt_image_bwd, mvlpt_image_fwd_begin / _resume and mvlpt_set_vpt_dropout return
 *     MVLPT_ERR_UNSUPPORTED with a message, without touching the device;
 *   - mvlpt_set_precision accepts all three modes; the ResNet tower runs single fp16 operands in each of them (it carries no
 *     gradient); the text tower, the heads, the cross-entropy, nearest-token and preprocess entries work as on any handle. */
typedef struct MvlptResNetArch {
  int image_resolution, width;
  int layers[4];
  int heads, output_dim;
} MvlptResNetArch;
int mvlpt_create_resnet(const MvlptArch* arch, const MvlptResNetArch* rn, void** handle);
/* switch the precision mode (takes effect at the next tower forward) */
int mvlpt_set_precision(void* handle, int mode);
/* The activation of the MLP in every transformer block of both towers (the text tower of a ResNet handle included).
 *   MVLPT_ACT_QUICKGELU  (default) x * sigmoid(1.702 x), clip/model.py:162-164: the archives clip.load downloads.  Fused into the
 *                        epilogues of the two MLP GEMMs.
 *   MVLPT_ACT_GELU       nn.GELU, the erf form x * Phi(x): CLIP checkpoints of the same architecture and the same state-dict keys
 *                        that were trained with it.  The MLP-up GEMM stores its fp32 pre-activation and a stand-alone pass applies
 *                        GELU (backward: GELU' on the fp32 dA) and writes the next GEMM's operand: two more element-wise passes
 *                        over [tokens, 4 width] per block and direction, and one fp32 scratch buffer of that size per tower
 *                        (plus [rows, 4 width] for the compact last block), counted by mvlpt_text_workspace_bytes only under this
 *                        setting.  The image tower's packed residual stream is not taken, and ln_2 is not folded into the
 *                        MLP-up GEMM (ln_1 still is).  Nothing else changes; MvlptArch does not carry the setting.
 * A setting like mvlpt_set_precision: legal before the first tower forward and after any completed step.  Between a forward with
 * save_for_bwd = 1 and the backward of that tower (and between mvlpt_image_fwd_begin and _resume) it returns MVLPT_ERR_STATE with a
 * message and changes nothing: the saved pre-activations belong to the activation of their forward.  Any other value:
 * MVLPT_ERR_ARG, nothing is touched. */
enum { MVLPT_ACT_QUICKGELU = 0, MVLPT_ACT_GELU = 1 };
int mvlpt_set_activation(void* handle, int activation);
int mvlpt_get_activation(void* handle, int* activation);
/* LayerNorm folding (no counterpart in the reference, which calls nn.LayerNorm as its own op, clip/model.py:186-187): inside a
 * tower the GEMM in front of a LayerNorm (out-projection / MLP down-projection + fp32 residual) also writes round16(x * gamma)
 * and per-row partial sums, and the GEMM behind it (QKV / MLP up-projection) applies mean and rstd in its epilogue — the
 * stand-alone LayerNorm pass over the residual stream disappears.  mode 0: off, 1: image tower, 2: both towers (default;
 * environment MVLPT_LN_FOLD); towers with fewer than `min_rows` token rows (default 4096) keep the stand-alone kernel. */
int mvlpt_set_ln_fold(void* handle, int mode, int min_rows);
/* Packed residual stream (ON by default since round 6; environment MVLPT_RESID_PACKED = 0 switches it off): an fp16 image tower that has
 * no prompt rows and keeps nothing for a backward (the CoOp configurations, BASELINE configs[0..1]; clip/model.py:185-188 `x = x + ...`)
 * carries the residual stream as hi = round16(x) + one byte with the next 8 bits of x instead of fp32, and hi is at the same time the
 * 16-bit operand of the GEMM behind every LayerNorm (its gamma folded into the frozen weight): 6 instead of 10 bytes of memory
 * traffic per element and residual update, x carried to 2^-20 (|x| saturates at 65504); image tower alone -1.7 %, headline step -0.9 %.
 * Round 5 kept it off because ~1 tower in 1 000 - 6 000 returned ONE image 1e-3 off under a concurrent text tower: that was the gfx950
 * packed-fp32 hazard in the tower entry kernel (NOTES_experiments.md round 6), gone since the library is built without packed fp32
 * instructions: 0 in 20 000 towers.  0: the fp32 stream everywhere. */
int mvlpt_set_resid_packed(void* handle, int on);
/* `vpt_dropout` of the reference (trainers/mvlpt.py:165, 424 and :77): the visual prompt rows are expanded over the batch and THEN
 * dropped out, so every image has its own mask.  masks = fp32 [n_layers, B, n_vpt, width] on the device, 0 or 1 / (1 - p): layer 0
 * belongs to the shallow prompts, layer l >= 1 to the deep prompts spliced in front of block l.  ONE-SHOT: the NEXT mvlpt_image_fwd
 * checks the extents against its own (n_layers >= 1 + n_deep, batch, n_vpt; a mismatch is MVLPT_ERR_ARG), multiplies the prompt rows
 * it writes with the masks, hands the pointer to ITS mvlpt_image_bwd (which multiplies the gradients it sums over the batch) and
 * clears the setting — a later forward without a new call runs without dropout.  The caller keeps the buffer alive until that
 * backward.  masks = NULL clears a pending setting. */
int mvlpt_set_vpt_dropout(void* handle, const float* masks, int n_layers, int batch, int n_vpt, int width);
/* Workspaces only grow, and a block that was outgrown is retired (not freed) so that no step ever meets a device-wide sync.
 * mvlpt_trim synchronises the device and releases the retired blocks: call it at an epoch boundary (e.g. after a one-off large
 * evaluation batch or class list). */
int mvlpt_trim(void* handle);
/* DEBUG (tools/tower_stage_probe.py; off by default, no cost when off): while enabled, mvlpt_image_fwd adds one 64-bit fingerprint
 * (position-weighted sum of the 32-bit words) per intermediate — patches, patch embedding, token assembly, and per packed block qkv,
 * attention output, the stream + row statistics behind each of the two updates, the MLP activations — to a device array it clears at
 * its start.  The call synchronises the device, copies up to max_out fingerprints of the LAST forward to host_out (may be NULL),
 * switches the recording on / off and returns the number copied.  Two runs on the same input agree entry by entry; the first entry
 * that differs names the kernel. */
int mvlpt_debug_checksums(void* handle, int enable, unsigned long long* host_out, int max_out);
int mvlpt_destroy(void* handle);
const char* mvlpt_last_error(void* handle); /* handle may be NULL for create() failures */
const char* mvlpt_version(void);

/* Streams confined to a partition of the compute units.  The reference runs the two towers one after the other on one
 * stream (`image_features = self.image_encoder(...)`, `text_features = self.text_encoder(...)`, trainers/mvlpt.py:543-548);
 * here they are independent until the logits and run side by side.  The image tower's persistent GEMM workgroups hold
 * every CU they are given for the whole launch, so the text tower's short, wide kernels would only ever run in their
 * tails: a stream from mvlpt_stream_create_cus owns logical compute units [cu_first, cu_first + cu_count)
 * (hipExtStreamCreateWithCUMask; logical CU i sits on XCD i % 8, so a multiple of 8 is the same share of every XCD), and
 * every launcher of this library sizes persistent / grid-stride grids by the stream's partition (mvlpt_stream_cus: the
 * partition size, or the device's CU count for any other stream).  Any hipStream_t still works everywhere. */
int mvlpt_stream_create_cus(int cu_first, int cu_count, mvlpt_stream_t* stream);
int mvlpt_stream_destroy(mvlpt_stream_t stream);
int mvlpt_stream_cus(mvlpt_stream_t stream);
/* Grid cap of ANY stream (no CU mask, no new stream): while it is set, mvlpt_stream_cus(stream) is min(partition size or device
 * count, n rounded DOWN to a multiple of 8 — workgroup b runs on XCD b % 8 and the tile remap of the persistent kernels assumes the
 * same share of every XCD), so the persistent / grid-stride launches enqueued on `stream` occupy at most that many compute units and
 * leave the rest to the kernels of other streams.  n <= 0 clears it; 1 .. 7 is MVLPT_ERR_ARG.  Results do not depend on the cap: the
 * GEMM geometries agree bit for bit, and where two kernels do not (the persistent attention forward against one workgroup per head)
 * the choice is made by the uncapped count.  Read on the host at enqueue time: setting and
 * clearing it between two enqueues needs no device synchronisation and does not touch launches already enqueued.  The NULL stream
 * cannot be capped (MVLPT_ERR_ARG). */
int mvlpt_stream_set_cu_cap(mvlpt_stream_t stream, int n);

/* Frozen weights (replaces `self.model.to(self.device)` for the CLIP towers, trainers/mvlpt.py:867, with a
 * one-time pack: 16-bit copy for the forward GEMM and a pre-transposed copy for the dX GEMM — legal because
 * every non-prompt parameter is frozen, trainers/mvlpt.py:855-858).  `name` is the key of
 * clip.model.CLIP.state_dict() ("visual.conv1.weight", "transformer.resblocks.3.mlp.c_fc.bias", ...).
 * `dev_ptr` is a contiguous device tensor of `dtype` (fp32/fp16/bf16).  Unknown names return MVLPT_ERR_ARG. */
int mvlpt_load_frozen(void* handle, const char* name, const void* dev_ptr, int dtype, const int64_t* shape, int ndim,
                      mvlpt_stream_t stream);
/* "token_embedding.weight" [vocab, text_width] is optional: when passed, an fp32 copy is kept for mvlpt_text_encode_tokens (vocab *
 * text_width * 4 bytes: 101 MB for ViT-B/16); callers that feed prefix / suffix embeddings skip the key and pay nothing.
 * 0 when every tensor the towers need has been loaded; otherwise <0 and last_error names the first missing. */
int mvlpt_frozen_ready(void* handle);

/* What the engine remembers of a forward.  It keeps one record per job (image tower, text tower, head): the last forward of that
 * job.  A backward, mvlpt_image_fwd_resume and mvlpt_set_activation decide by it alone, and a forward that returns an error after it
 * has touched the job's workspace leaves nothing a backward would run on: the backward then returns MVLPT_ERR_STATE.  A forward
 * refused for its arguments before that point leaves the record of the forward in front of it usable.
 * Every input of a forward is read by the launches it enqueues.  These caller buffers are read AGAIN by later calls, so they stay
 * valid and unchanged for longer:
 *   - the masks of mvlpt_set_vpt_dropout: from the mvlpt_image_fwd (or _begin) that takes them over until its last mvlpt_image_bwd
 *     has been enqueued;
 *   - vpt_deep (and vpt, and the masks) of mvlpt_image_fwd_begin: until mvlpt_image_fwd_resume has been enqueued;
 *   - ctx_deep of a saving mvlpt_text_fwd: until its last mvlpt_text_bwd has been enqueued;
 *   - task_lo / task_hi of mvlpt_logits_fwd: until the last mvlpt_logits_bwd of that forward has been enqueued.
 * The class ranges of the ranged entries are host arrays, copied by the call. */

/* ImageEncoder.forward (trainers/mvlpt.py:52-93).  image [B,3,R,R] of `image_dtype`; vpt [n_vpt,dv] fp32 or
 * NULL (shallow prompts, forward_vpt :416-437); vpt_deep [n_deep,n_vpt,dv] fp32 or NULL (deep prompts for
 * layers 1..n_deep, :73-83).  feat_out [B,embed] fp32.  save_for_bwd != 0 keeps activations for image_bwd. */
int mvlpt_image_fwd(void* handle, const void* image, int image_dtype, const float* vpt, const float* vpt_deep, int n_vpt,
                    int n_deep, int B, float* feat_out, int save_for_bwd, mvlpt_stream_t stream);
/* The same forward in two enqueues (mvlpt_image_fwd is begin(stop_block = layers) + resume): begin carves the workspace and runs the
 * tower entry and blocks [0, stop_block) (clamped to [0, layers]; the CLS-only last block always belongs to resume); resume runs
 * blocks [stop_block, layers), ln_post and the projection into feat_out [B,embed], on a stream of the caller's choice — ordering the
 * two streams is the caller's job.  The launches, their order and (on equally sized grids) their results are those of
 * mvlpt_image_fwd.  The engine holds ONE pending forward: resume without begin, a second begin before resume and mvlpt_image_bwd in
 * between return MVLPT_ERR_STATE without touching the device.  vpt / vpt_deep and the dropout masks must stay valid until resume has
 * been enqueued.  mvlpt_image_fwd_abandon forgets a pending begin (its workspace is reused by the next begin; host state only). */
int mvlpt_image_fwd_begin(void* handle, const void* image, int image_dtype, const float* vpt, const float* vpt_deep, int n_vpt,
                          int n_deep, int B, int save_for_bwd, int stop_block, mvlpt_stream_t stream);
int mvlpt_image_fwd_resume(void* handle, float* feat_out, mvlpt_stream_t stream);
int mvlpt_image_fwd_abandon(void* handle);
/* dX-only backward of the image tower: dfeat [B,embed] fp32 -> dvpt [n_vpt,dv], dvpt_deep [n_deep,n_vpt,dv]
 * (sum over the batch: prompts are `expand`ed, :75,:424).  Must follow image_fwd(save_for_bwd=1), same B. */
int mvlpt_image_bwd(void* handle, const float* dfeat, float* dvpt, float* dvpt_deep, mvlpt_stream_t stream);

/* One text forward over prompts: forward_coop + TextEncoder.forward (trainers/mvlpt.py:439-515, 105-130).  The kind follows from the
 * fields: class_lo / class_hi set = ranged, n_deep > 0 = deep, otherwise plain.  Pointers first, fixed-width fields, no implicit padding;
 * a zeroed struct with the fields of one kind filled in by name is a valid job.  Device pointers unless marked HOST. */
typedef struct MvlptTextJob {
  /* the class tables: prefix [n_cls,1,dt], suffix [n_cls,L-1-n_ctx,dt] fp32 (the `token_prefix` / `token_suffix` buffers, :312-316) */
  const float* prefix;
  const float* suffix;
  /* plain: [n_ctx,dt] (ctx_per_class = 0) or [n_cls,n_ctx,dt] (CSC, ctx_per_class = 1) fp32, NULL when n_ctx == 0; deep: [n_ctx,dt];
   * ranged: [groups,n_ctx,dt], one context block per image (ctx + meta_net(image g)), n_ctx > 0 */
  const float* ctx;
  /* Deep language prompting (per-layer text contexts; the language half of MaPLe, "independent V-L prompting" next to deep visual
   * prompts): [n_deep,n_ctx,dt] fp32.  In front of block l = 1 .. n_deep the hidden states at the context positions are replaced,
   * x_l[c, ctx_pos[c,j], :] = ctx_deep[l-1, j, :], for every class c and every CLASS_TOKEN_POSITION (the positions come from `layout`).
   * No positional embedding is added to the replaced rows.  Blocks behind n_deep run on whatever the block in front of them left; no
   * block is skipped.  ln_1 of a block behind an overwrite is not folded into the FC2 in front of it (n_deep more LayerNorm launches
   * when LayerNorm folding is on).  Ignored when n_deep == 0: the launches and the bits of the plain tower.  With save_for_bwd it stays
   * valid and unchanged until the backward has been enqueued on the same stream: under mvlpt_set_text_act_ckpt the backward's
   * recomputation of a segment reads it again. */
  const float* ctx_deep;
  /* int32 [n_cls,L]: source row per position — 0 = prefix, e>0 = suffix row e-1, e<0 = ctx row -e-1 (encodes the end/middle/front layouts) */
  const int32_t* layout;
  /* int32 [n_cls] = argmax of tokenized_prompts (:128) */
  const int32_t* eot;
  /* HOST int32 [groups], both NULL unless ranged (the task of an image is known on the host before the step); checked and uploaded with
   * the call, which stays enqueue-only.  Group g owns classes [class_lo[g], class_hi[g]), 0 <= lo <= hi <= n_cls (an empty range is
   * legal, not all of them); its sequences are those classes in order, each class c's prefix / suffix / layout row / eot with context
   * block g, the groups follow one another as ONE tower: S = sum_g (hi - lo) sequences, S * L inside int32.  The class tables are read
   * through the ranges, never copied.  The MVLPT trainer's CoCoOp branch under MULTITASK_LABEL_PERTASK (trainers/mvlpt.py:556-581): image
   * g keeps only the logits of its own task's class range, so only those sequences run.  Every range [0, n_cls) is CoCoOp's tower,
   * PromptLearner.forward + one TextEncoder call per image (trainers/cocoop.py:123-161, 48-59): row g * n_cls + c = (image g, class c). */
  const int32_t* class_lo;
  const int32_t* class_hi;
  int32_t n_ctx;         /* context tokens, 0 <= n_ctx <= L - 2 */
  int32_t ctx_per_class; /* plain only */
  int32_t n_deep;        /* 0 <= n_deep <= text_layers - 1 (block 0 reads the embedding-level context); > 0 needs n_ctx > 0 and ctx_deep */
  int32_t groups;        /* ranged: 1 .. 65535; 0 otherwise */
  int32_t n_cls;         /* rows of the class tables */
  int32_t L;             /* L <= context_length (CUT_CONTEXTLEN gives L < 77, :111-117) */
  int32_t save_for_bwd;  /* != 0 keeps activations for mvlpt_text_bwd */
  int32_t reserved;      /* 0 */
} MvlptTextJob;
#define MVLPT_TEXT_JOB_BYTES 96
/* feat_out [n_cls,embed] fp32 ([S,embed] ranged).  MVLPT_ERR_ARG before any device work or engine state is touched: a null table, a
 * field outside the limits above, class_lo / class_hi / groups not all set or all clear, and the combinations that are not offered:
 * deep prompts with ctx_per_class or on the ranged tower, ctx_per_class on the ranged tower.  mvlpt_text_workspace_bytes does not depend
 * on the kind. */
int mvlpt_text_fwd(void* handle, const MvlptTextJob* job, float* feat_out, mvlpt_stream_t stream);
/* dfeat [n_cls,embed] fp32 -> dctx (same shape as ctx).  Must follow mvlpt_text_fwd with save_for_bwd and n_ctx > 0.  Ranged: dfeat
 * [S,embed] -> dctx [groups,n_ctx,dt], dctx[g] = sum over the sequences of group g's own range in a fixed order (no atomics:
 * deterministic); all zeros for an empty range.  dctx_deep [n_deep,n_ctx,dt] exactly when the forward had n_deep > 0, NULL otherwise
 * (MVLPT_ERR_ARG either way round; the saved forward stays usable): dctx_deep[l-1, j] = sum over the classes (fixed order, no atomics)
 * of the gradient at the input of block l at ctx_pos[c,j]; those rows then carry no gradient into block l-1. */
int mvlpt_text_bwd(void* handle, const float* dfeat, float* dctx, float* dctx_deep, mvlpt_stream_t stream);
/* *out = bytes of text-tower workspace a mvlpt_text_fwd (S sequences when ranged) over C_total sequences of length L reserves (the
 * ctx-position table counted for the largest n_ctx, L - 2; a ranged tower adds its range tables and a per-class
 * position table, a few bytes per class and sequence, which the figure covers unless n_ctx is within a few tokens of L - 2); the
 * workspace only grows, so a caller that chunks G keeps its peak under a budget.  With save_for_bwd the figure is the one under the
 * current mvlpt_set_text_act_ckpt setting (below): fewer saved layers, more sequences per chunk. */
int mvlpt_text_workspace_bytes(void* handle, int C_total, int L, int save_for_bwd, int64_t* out);
/* Activation checkpointing of the text tower, TRAINER.ACT_CKPT of the reference (trainers/mvlpt.py:119-121:
 * checkpoint_sequential(resblocks, ACT_CKPT, x)).  An engine setting like mvlpt_set_precision; default 1 (everything saved).
 * The plan is torch's: k = min(segments, text_layers) segments, the first k - 1 of text_layers / k blocks each, the last one takes
 * the rest.  A saving forward (mvlpt_text_fwd of any kind with save_for_bwd = 1) keeps only the input of the first k - 1 segments
 * and the activations of the last one; mvlpt_text_bwd runs every other segment again before that segment's backward, launch for launch
 * as the forward did (no LayerNorm is folded across a segment boundary: k - 1 more LayerNorm launches), so features and dctx have
 * the bits of an un-checkpointed tower whenever LayerNorm folding is off or the tower is below its row threshold, and stay within
 * the tower's accuracy otherwise.  The largest segment is the last one, text_layers - (k - 1) * (text_layers / k) blocks, which is
 * not monotonic in k (12 layers: k = 5 -> 4 blocks, k = 7 -> 6 blocks); k in {2, 3, 4, 6, 12} are the useful settings at 12 layers.
 * segments < 1: MVLPT_ERR_ARG.  Takes effect at the next text forward and in mvlpt_text_workspace_bytes, which reports the reduced
 * figure; a forward records its own plan, so a call between a forward and its backward does not change that backward.  With k > 1 a
 * backward consumes the saved state: a second mvlpt_text_bwd on the same forward returns MVLPT_ERR_STATE without launching (with
 * k = 1 it still repeats the backward).  mvlpt_text_encode_tokens and the image tower save nothing and are not affected. */
int mvlpt_set_text_act_ckpt(void* handle, int segments);
/* The plan the next saving text forward will use under the current setting (trainers/mvlpt.py:119-121, torch's
 * checkpoint_sequential rule as above): *n_segments = k, first_layer[i] = first block of segment i for i < k (HOST array of `cap`
 * entries; cap < k: MVLPT_ERR_ARG, *n_segments still set).  Segments 0 .. k-2 are checkpointed, segment k-1 is saved. */
int mvlpt_text_act_ckpt_plan(void* handle, int32_t* first_layer, int cap, int* n_segments);
/* Gradient length of the text tower: the backward processes only the leading grad_len positions of every sequence.  The only
 * gradient entering the tower sits on each sequence's EOT row, the attention is causal and LayerNorm, MLP and activation act row by
 * row, so in every block the gradient of a position behind its sequence's EOT is exactly 0.0: with max(eot) < grad_len the backward
 * skips rows of zeros and dctx / dctx_deep keep their bits.  The forward is untouched (every position is evaluated and saved, at the
 * pitch L); the gradient buffers are compact [C, grad_len, .].  An engine setting like mvlpt_set_text_act_ckpt; the default is every
 * position.  grad_len outside [MVLPT_TEXT_MIN_L, context_length] or max_eot < 0: MVLPT_ERR_ARG.  Takes effect at the next saving
 * text forward (plain, deep or ranged), which runs under min(grad_len, L) and records it, so a call between a forward and its
 * backward does not change that backward.  max_eot is the CALLER'S largest entry of the `eot` tables it will pass (a device array
 * the engine does not read back): a saving forward whose gradient length is below L and not above max_eot returns MVLPT_ERR_ARG before
 * anything is launched, and a caller whose tables change calls this again.  An understated max_eot gives a wrong gradient, never an
 * out-of-bounds access.  mvlpt_text_workspace_bytes keeps reporting the figure of the full length, an upper bound. */
int mvlpt_set_text_grad_len(void* handle, int grad_len, int max_eot);
/* Shared prefix of the class prompts: the CALLER vouches that positions 0 .. prefix-1 of `layout` hold the same entries in every class
 * row, none of them a suffix entry, that every row of `prefix` (the SOS embedding) is bitwise the same, that the context is generic and
 * that every EOT lies at or behind position `prefix`.  The attention is causal and everything else acts row by row, so those positions
 * have the same hidden state in every sequence: the tower evaluates them once, in C + 1 "slots" of L - P rows (slot 0: the prefix,
 * slot c + 1: positions P .. L-1 of class c), and its backward carries the SUM over the classes of their gradient, which is all dctx
 * needs; the one class-dependent path into them, dK / dV of the prefix keys from later queries, is summed from fp32 partials in a fixed
 * order (no atomics).  For more than 512 classes that sum is carried scaled down by a power of two and rescaled exactly at the end.
 * The features keep their bits; dctx rows of prefix positions change at rounding level (another summation order).
 * Unlike mvlpt_set_text_grad_len the engine cannot check this setting against its tables, so it is ONE-SHOT: the next text forward
 * through either entry (mvlpt_text_fwd of any kind, saving or not; mvlpt_text_encode_tokens) consumes it, and a forward without a new
 * call runs without a prefix.  The forward records what it ran under: a call between a forward and its backward does not change that
 * backward.  0 (the default): off, today's launches.  prefix < 0 or >= context_length: MVLPT_ERR_ARG.  The engine uses
 * P = min(prefix, L - 1) lowered until P <= grad_len - P and grad_len - P >= MVLPT_TEXT_MIN_L (any shorter prefix is as correct), and
 * P = 0 on every route that has no slot layout: ctx_per_class, deep prompts, the ranged and token-id entries, activation checkpointing
 * (mvlpt_set_text_act_ckpt > 1), L > 80.  Split and single operands (MVLPT_PREC_FAST) share alike.  mvlpt_text_workspace_bytes keeps reporting the
 * figure without a prefix: an upper bound once the prefix saves rows ((C + 1) (L - P) + the partials <= C L); the workspace grows on
 * demand otherwise. */
int mvlpt_set_text_shared_prefix(void* handle, int prefix);

/* CLIP.encode_text (clip/model.py:343-356: token_embedding(text) + positional_embedding -> transformer -> ln_final ->
 * x[arange, text.argmax(-1)] @ text_projection) for S sequences of token ids: what the zero-shot trainers feed (trainers/zsclip.py:45-49,
 * 91-92).  Needs "token_embedding.weight" [vocab, text_width], which mvlpt_load_frozen keeps as an fp32 copy when (and only when) the
 * caller passes it; mvlpt_frozen_ready does not ask for it.
 * ids is a HOST int32 [S, ld] array, ld >= L; the device reads columns 0 .. L-1 only (the tower is causal: positions behind the EOT
 * token cannot reach the EOT row, so trimming a sequence to L > eot is exact, not an approximation).  The table is checked on the host
 * and uploaded with the call, which stays enqueue-only; nothing is launched when the check fails:
 *   - any id in columns 0 .. L-1 outside [0, vocab): MVLPT_ERR_ARG (it would be an out-of-bounds read of the table);
 *   - a row whose EOT position — first occurrence of the maximum of the WHOLE row of ld ids, as text.argmax(dim=-1) — is >= L;
 *   - L > context_length, or L < MVLPT_TEXT_MIN_L: the attention and GEMM launchers take any L >= 1 (any M >= 1), the tower needs
 *     L >= n_ctx + 2 = 2, and mvlpt_text_workspace_bytes, which sizes it, refuses L <= 2 — so 3 is the smallest L every entry accepts;
 *   - S > 65535 (the attention launches put the sequence index on grid.y; callers chunk, as they do for the workspace);
 *   - no token embedding loaded: MVLPT_ERR_STATE.
 * feat_out [S, embed] fp32, un-normalised.  Workspace: mvlpt_text_workspace_bytes(S, L, 0) plus the id table,
 * ((S * L + S) * 4 rounded up to 256) bytes (the trimmed ids and one EOT row index per sequence).  Everything behind the assembly is
 * the tower of mvlpt_text_fwd with n_ctx = 0, save_for_bwd = 0: the same bits for the same embeddings.  No gradient on this route. */
enum { MVLPT_TEXT_MIN_L = 3 };
int mvlpt_text_encode_tokens(void* handle, const int32_t* ids, int ld, int S, int L, float* feat_out, mvlpt_stream_t stream);
/* Prompt ensembling (trainers/zsclip.py:88-96) as one kernel: feats fp32 [T, C, e], template-major as the reference loops;
 * out[c] = normalize((1/T) * sum_t feats[t,c] / |feats[t,c]|), fp32, summed over t in the fixed order 0 .. T-1 (reruns are
 * bit-identical).  T = 1 gives x / |x| with the bits of the head's row normalisation (the mean of one unit vector is that vector; the
 * second normalisation is skipped).  e <= 1024.  Handle-free: errors go to mvlpt_last_error(NULL). */
int mvlpt_text_ensemble(const float* feats, int T, int C, int e, float* out, mvlpt_stream_t stream);

/* Cosine logits (trainers/mvlpt.py:550-554) with the multiplicative per-task mask (:573-581):
 * logits[b,c] = exp(logit_scale) * <img_b/|img_b|, txt_c/|txt_c|> * [task_lo[b] <= c < task_hi[b]].
 * task_lo/task_hi int32 [B] or NULL (no mask).  fp32 throughout. */
int mvlpt_logits_fwd(void* handle, const float* img_feat, const float* txt_feat, float logit_scale_exp, const int32_t* task_lo,
                     const int32_t* task_hi, int B, int C, float* logits, mvlpt_stream_t stream);
/* dlogits [B,C] -> dimg [B,embed], dtxt [C,embed] (either may be NULL).  Uses the features of the last
 * mvlpt_logits_fwd call on this handle. */
int mvlpt_logits_bwd(void* handle, const float* dlogits, float* dimg, float* dtxt, mvlpt_stream_t stream);
/* The ranged head: img [G,embed], txt [S,embed] (rows of a ranged mvlpt_text_fwd over the same HOST class_lo / class_hi), logits [G,C]:
 * inside image g's range the cosine logit against its own text row, outside it exactly 0.0f (logits * select_index, :581).
 * The backward reads dlogits [G,C] inside the ranges only and gives dtxt [S,embed] and / or dimg [G,embed] (either may be NULL): dimg is
 * the gradient with respect to the UN-normalised image features (the image tower may carry visual prompts on this route).  Uses the
 * features of the last logits_ranged_fwd on this handle; after mvlpt_logits_fwd it returns MVLPT_ERR_STATE, as mvlpt_logits_bwd does
 * after logits_ranged_fwd.  fp32 throughout.
 * Every range [0, C) is CoCoOp's head (trainers/cocoop.py:184-189): logits[g,c] = logit_scale_exp * <img_g/|img_g|,
 * txt_{gC+c}/|txt_{gC+c}|> over txt [G*C,embed]; its backward asks for dtxt only (dimg NULL: the image tower is frozen and carries no
 * prompts there). */
int mvlpt_logits_ranged_fwd(void* handle, const float* img, const float* txt, float logit_scale_exp, const int32_t* class_lo,
                            const int32_t* class_hi, int G, int C, float* logits, mvlpt_stream_t stream);
int mvlpt_logits_ranged_bwd(void* handle, const float* dlogits, float* dtxt, float* dimg, mvlpt_stream_t stream);

/* F.cross_entropy(output, label) with mean reduction (trainers/mvlpt.py:931) and its gradient.
 * labels: int64 [B] (MVLPT_LABEL_INT64) or fp32 probabilities [B,C] (MVLPT_LABEL_PROB_F32, rows already
 * normalised as in :914-916).  loss [1]; dlogits [B,C] or NULL; ncorrect [1] or NULL (top-1 hits, with
 * argmax(label) as the target for soft labels, :935-936). */
int mvlpt_cross_entropy(void* handle, const float* logits, const void* labels, int label_kind, int B, int C, float* loss,
                        float* dlogits, float* ncorrect, mvlpt_stream_t stream);

/* ---- kernel-level entry points (what the parity tests call; same kernels the towers use) ------------------ */
/* C[M,N] = A[M,K] * Bt[N,K]^T with epilogue `epi` (0 store16(+bias), 1 bias+QuickGELU (out2 = pre-activation),
 * 2 fp32 out = acc+bias+resid32, 3 out16 = acc*QuickGELU'(aux16), 4 fp32 store).  K % 64 == 0, N % 128 == 0. */
int mvlpt_op_gemm(int dtype, int epi, const void* A, const void* Bt, int M, int N, int K, const float* bias, const void* aux,
                  const float* resid, void* out, void* out2, mvlpt_stream_t stream);
/* The same launch with every GEMM argument the towers set: a_split (0 single, 1 hi|lo pair, 2 mixed pair: A rows as described
 * below), row pitches in 16-bit elements lda (A; 0 = dense: K, or 2K for a pair), ldo (`out` of the pair-producing epilogues 5 / 6 /
 * 7; 0 = dense: 2N) and ldb (Bt; 0 = K), w8_exp (mixed pair: exponent of the weight's fp8 plane) and out_lo8 (epilogues 5 / 6: the
 * output is a mixed pair instead of a hi|lo pair).  Pitches are multiples of 8 elements; an illegal combination returns an error. */
int mvlpt_op_gemm_ex(int dtype, int epi, const void* A, const void* Bt, int M, int N, int K, const float* bias, const void* aux,
                     const float* resid, void* out, void* out2, int a_split, int lda, int ldo, int ldb, int w8_exp, int out_lo8,
                     mvlpt_stream_t stream);
/* The stand-alone activation pass of MVLPT_ACT_GELU, kernel level (both are also instantiated for MVLPT_ACT_QUICKGELU, which the
 * engine never takes: it reproduces epilogues 1 / 5 bit for bit from the fp32 pre-activation epilogue 4 stores).
 *   forward:  out = act(u32), u16_out (optional, 16-bit [M, N] dense) = u32 rounded once;
 *   backward: out = da32 * act'(u16), u16 the saved pre-activation (16-bit [M, N] dense).
 * u32 / da32: fp32 [M, N] at a pitch of ld_in floats (0 = dense).  `out` is the A operand of the next GEMM in out_format
 * MVLPT_ACT_OUT_SINGLE (16-bit [M, N]), _PAIR (hi|lo pair [M, 2N]) or _MIXED (mixed pair, [hi | e5m2 residual bytes | unused], same
 * pitch) at a pitch of ld_out 16-bit elements (0 = dense: N, or 2N for the pairs).  dtype: MVLPT_DT_F16 / _BF16, the 16-bit type.
 * N and both pitches are multiples of 8, every pointer is 16-byte aligned, M is arbitrary.  An unknown activation or format, a pitch
 * below the row width or not a multiple of 8, a null or misaligned pointer: MVLPT_ERR_ARG, nothing is launched or written. */
enum { MVLPT_ACT_OUT_SINGLE = 0, MVLPT_ACT_OUT_PAIR = 1, MVLPT_ACT_OUT_MIXED = 2 };
int mvlpt_op_activation_fwd(int dtype, int activation, const float* u32, int ld_in, int M, int N, int out_format, void* out, int ld_out,
                            void* u16_out, mvlpt_stream_t stream);
int mvlpt_op_activation_bwd(int dtype, int activation, const float* da32, int ld_in, const void* u16, int M, int N, int out_format,
                            void* out, int ld_out, mvlpt_stream_t stream);
/* Which kernel a GEMM launch on `stream` would use, without launching (the choice depends on the tile counts against the stream's
 * compute units; fold_ntp > 0: a folded consumer, mvlpt_op_gemm_folded, with that many slots per row).  Returns the kernel family
 * (MVLPT_GEMM_*) and its tile / LDS-ring depth through the optional pointers, or a negative error. */
enum { MVLPT_GEMM_BT_128x128_R2 = 1, MVLPT_GEMM_BT_128x128_R4 = 2, MVLPT_GEMM_BT_256x128_R3 = 3, MVLPT_GEMM_BT_256x256_R2 = 4,
       MVLPT_GEMM_PHASED = 5, MVLPT_GEMM_PC = 6, MVLPT_GEMM_PCP = 7 };
int mvlpt_op_gemm_route(int dtype, int epi, int a_split, int M, int N, int K, int fold_ntp, mvlpt_stream_t stream, int* tile_m,
                        int* tile_n, int* ring);
/* same with a split-precision A operand: A is [M, 2K] = [A_hi | A_lo] (16-bit pair), C = (A_hi + A_lo) * Bt^T; additional
 * epilogues 5 (out [M,2N] = hi|lo pair of QuickGELU(acc+bias), out2 = pre-activation) and 6 (pair of acc*QuickGELU'(aux)).
 * Note: the saved pre-activation `out2` is ONE 16-bit value per element in every mode (QuickGELU' is evaluated on it in the
 * backward): the one operand of the split towers that is not a pair; the parity budget carries it (gradients 1-7e-4 of 1e-3). */
int mvlpt_op_gemm_split(int dtype, int epi, const void* A, const void* Bt, int M, int N, int K, const float* bias, const void* aux,
                        const float* resid, void* out, void* out2, mvlpt_stream_t stream);
/* LayerNorm with the 16-bit output written as a hi|lo pair [rows, 2d] */
int mvlpt_op_layernorm_fwd_split(int out_dtype, const float* x, const float* gamma, const float* beta, void* y, int rows, int d,
                                 mvlpt_stream_t stream);
int mvlpt_op_layernorm_bwd_split(int dtype, const void* dy, const float* x, const float* gamma, const float* resid, float* out32,
                                 void* out16, int rows, int d, mvlpt_stream_t stream);
/* attention core of the split-precision mode; every operand is a 16-bit hi|lo pair [rows, 2*cols] = [hi(cols) | lo(cols)]:
 * qkv [N*L, 6*H*64] -> out [N*L, 2*H*64], lse;  backward: dout [N*L, 2*H*64] -> dqkv [N*L, 6*H*64] (delta: [N*H*L] scratch) */
int mvlpt_op_attention32_fwd(int dtype, const void* qkv, void* out, float* lse, int N, int L, int H, int causal, int q_rows,
                             mvlpt_stream_t stream);
int mvlpt_op_attention32_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                             void* dqkv, int N, int L, int H, int causal, mvlpt_stream_t stream);
/* ---- mixed pair: the default split format of MVLPT_PREC_SPLIT_GRAD.  A row holds [hi (cols x 16 bit) | residual bytes (cols) |
 * unused] at the pair's pitch of 2*cols 16-bit elements: hi = round16(x), byte = e5m2((x - hi) * 2^10) (bf16: 2^7).  A GEMM with
 * such an A operand multiplies hi with the 16-bit weight on v_mfma_f32_16x16x32 and the residual bytes with the weight's e4m3
 * copy on v_mfma_scale_f32_16x16x128_f8f6f4 (twice the rate): 1.5x the matrix time of a single-operand GEMM instead of 2x.
 * pack_weight_mixed: w32 [rows, cols] fp32 -> out [R, 3K/2] 16-bit elements = [W16 (K) | e4m3(W * 2^*w8_exp) (K bytes)] with
 * (R, K) = (rows, cols), or (cols, rows) when `transposed`; synchronises the stream (the exponent is returned to the host).
 * gemm_mixed: epilogues 2 / 4 (fp32 outputs), 7 (16-bit pair for the attention core), 5 / 6 (mixed-pair outputs). K % 128 == 0. */
int mvlpt_op_pack_weight_mixed(int dtype, const float* w32, int rows, int cols, int transposed, void* out, int* w8_exp,
                               mvlpt_stream_t stream);
int mvlpt_op_gemm_mixed(int dtype, int epi, const void* A, const void* Bt, int ldb, int w8_exp, int M, int N, int K, const float* bias,
                        const void* aux, const float* resid, void* out, void* out2, mvlpt_stream_t stream);
int mvlpt_op_cast_mixed(int dtype, const float* in, void* out, int64_t rows, int d, mvlpt_stream_t stream);
/* ---- LayerNorm folding at kernel level (see mvlpt_set_ln_fold): LN(x) W^T + b = rstd_r (x gamma) W^T - rstd_r mean_r (W gamma) + (b + W beta).
 * fold_vectors: colsum = W gamma, bias2 = b + W beta from the PACKED 16-bit weight W16 [N, ld] (load time).
 * gemm_ln_producer: out32 = A Bt^T + bias + resid (as epilogue 2) AND x16 = round16(out32 * gamma) in the A-operand format
 *   x16_split (0 [M,N], 1 hi|lo pair [M,2N], 2 mixed pair) AND part[(row * ntp + j) * 2 ..] = {sum, sum of squares} of the row over
 *   output columns 128 j .. 128 j + 127, *nt = N / 128 slots whatever tile geometry the launch uses (ntp: slots per row, even, >= *nt, <= 8).  A: a_split 0 / 1 / 2 as in op_gemm*.
 * gemm_folded: epilogue `epi` (0, 1, 5, 7) on A16 = x16 with the normalisation applied from `part` (K = length of the rows). */
int mvlpt_op_fold_vectors(int dtype, const void* W16, int ld, const float* gamma, const float* beta, const float* b, float* colsum,
                          float* bias2, int N, int K, mvlpt_stream_t stream);
int mvlpt_op_gemm_ln_producer(int dtype, const void* A, int a_split, const void* Bt, int ldb, int w8_exp, int M, int N, int K,
                              const float* bias, const float* resid, const float* gamma, int x16_split, float* out32, void* x16,
                              float* part, int ntp, int* nt, mvlpt_stream_t stream);
int mvlpt_op_gemm_folded(int dtype, int epi, const void* A16, int a_split, const void* Bt, int ldb, int w8_exp, int M, int N, int K,
                         const float* colsum, const float* bias2, const float* part, int ntp, int nt, void* out, void* out2,
                         mvlpt_stream_t stream);
/* ---- packed residual stream at kernel level (see mvlpt_set_resid_packed; fp16 only).  An element x is stored as hi = round16(x)
 * and lo = clamp((bits(x) - bits(float(hi))) >> 5, -128, 127) (int8): x' = bits(float(hi)) + (lo << 5).
 * fold_weight: Wg = round16(W16 * gamma) [N, ldg], colsum = row sums of Wg (load time).  respk_pack: fp32 rows -> (hi, lo) and,
 *   when part != NULL, {sum, sum of squares} of each row in slot 0 of its ntp slots (the others 0).  respk_unpack: rows r * row_mul
 *   of (hi, lo) -> fp32.  gemm_residp: (hi_out, lo_out) = pack(A Bt^T + bias + unpack(hi_in, lo_in)) (in place allowed) and the
 *   row statistics of the fp32 value as in gemm_ln_producer; the consumer is gemm_folded on A16 = hi_out with Bt = Wg. */
int mvlpt_op_fold_weight(const void* W16, int ld, const float* gamma, void* Wg16, int ldg, float* colsum, int N, int K,
                         mvlpt_stream_t stream);
int mvlpt_op_respk_pack(const float* x, void* hi, uint8_t* lo, float* part, int ntp, int rows, int d, mvlpt_stream_t stream);
/* the tower entry of the packed stream (ImageEncoder.forward's class token + positional embedding + ln_pre, trainers/mvlpt.py:60-66,
 * straight into the packed format): rows [batch, 1 + grid2, d] from patch_emb [batch * grid2, d], cls [d], pos [1 + grid2, d];
 * part as in respk_pack (the statistics of block 0's ln_1) */
int mvlpt_op_assemble_packed(const float* patch_emb, const float* cls, const float* pos, const float* ln_g, const float* ln_b, void* hi,
                             uint8_t* lo, float* part, int ntp, int batch, int grid2, int d, mvlpt_stream_t stream);
int mvlpt_op_respk_unpack(const void* hi, const uint8_t* lo, int row_mul, float* out, int rows, int d, mvlpt_stream_t stream);
int mvlpt_op_gemm_residp(const void* A, const void* Bt, int ldb, int M, int N, int K, const float* bias, const void* hi_in,
                         const uint8_t* lo_in, void* hi_out, uint8_t* lo_out, float* part, int ntp, int* nt, mvlpt_stream_t stream);
int mvlpt_op_layernorm_fwd_mixed(int out_dtype, const float* x, const float* gamma, const float* beta, void* y, int rows, int d,
                                 mvlpt_stream_t stream);
int mvlpt_op_layernorm_bwd_mixed(int dtype, const void* dy, const float* x, const float* gamma, const float* resid, float* out32,
                                 void* out16, int rows, int d, mvlpt_stream_t stream);
/* attention core with 16-bit pair inputs (qkv, dout) and mixed-pair tensors on the GEMM side (out; dqkv) */
int mvlpt_op_attention32_fwd_mixed(int dtype, const void* qkv, void* out, float* lse, int N, int L, int H, int causal, int q_rows,
                                   mvlpt_stream_t stream);
int mvlpt_op_attention32_bwd_mixed(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                                   void* dqkv, int N, int L, int H, int causal, mvlpt_stream_t stream);
int mvlpt_op_layernorm_fwd(int out_dtype, const float* x, const float* gamma, const float* beta, void* y, int rows, int d,
                           mvlpt_stream_t stream);
int mvlpt_op_layernorm_bwd(int dtype, const void* dy, const float* x, const float* gamma, const float* resid, float* out32,
                           void* out16, int rows, int d, mvlpt_stream_t stream);
/* qkv [N*L,3*H*64] 16-bit -> out [N*L,H*64], lse [N*H*L] (may be NULL); heads of 64 (wider heads: mvlpt_op_attention_wide_fwd) */
int mvlpt_op_attention_fwd(int dtype, const void* qkv, void* out, float* lse, int N, int L, int H, int causal,
                           mvlpt_stream_t stream);
int mvlpt_op_attention_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                           void* dqkv, int N, int L, int H, int causal, mvlpt_stream_t stream);
/* The forward for heads wider than 64 (attention_wide.hip), non-causal, any L >= 1: qkv [N*L,3*H*w] 16-bit with head h at h*w inside
 * each third -> out [N*L,H*w], lse [N*H*L] (may be NULL), w = head_width in {80, 96, 112, 128} (any other: MVLPT_ERR_UNSUPPORTED; 64 is
 * mvlpt_op_attention_fwd's).  q_rows > 0: only queries 0..q_rows-1 of every sequence are computed and only their rows of out / lse are
 * written.  Scores are scaled by 1/sqrt(w) in fp32, the softmax runs online in fp32, P is rounded once to the 16-bit type, keys >= L
 * weigh exactly 0.  Handle-free and enqueue-only; a NULL pointer, a non-positive size or an unknown dtype returns MVLPT_ERR_ARG with
 * nothing launched.  There is no backward. */
int mvlpt_op_attention_wide_fwd(int dtype, const void* qkv, void* out, float* lse, int N, int L, int H, int head_width, int q_rows,
                                mvlpt_stream_t stream);
int mvlpt_op_cast(int dtype, const float* in, void* out, int64_t n, mvlpt_stream_t stream);
/* ---- LayerNorm, the operand-format kernels and the patch extraction with every argument the towers set (tests/test_hip_norm_matrix.py,
 * tests/test_hip_formats.py).  Every entry checks its arguments before anything is launched: a NULL pointer, an unknown dtype / format /
 * split returns MVLPT_ERR_ARG, a shape the kernels do not have (d % 4, d > 2048, Kp % 8, R % P) MVLPT_ERR_UNSUPPORTED, and the output is
 * untouched; rows = 0 succeeds and writes nothing.
 * layernorm_fwd_ex: y row r = LN(x row r * row_mul) (biased variance, eps 1e-5, fp32 statistics); out_dtype fp32 / fp16 / bf16; split
 *   (16-bit only) 0: y [rows, d], 1: hi|lo pair [rows, 2d], 2: mixed pair at the same pitch.
 * layernorm_bwd_ex: dy [rows, d] dense, of dy_dtype (fp32: what the towers pass; or `dtype`); row r of x, resid, out32 and out16 is row
 *   r * row_mul of its buffer (the rows in between are not touched): out32 = (resid ? resid : 0) + dLN/dx, out16 = out32 in the format
 *   `split`.  resid and out16 may be NULL, out32 may alias resid.
 * layernorm_route: which kernel both of them run for rows x d on `stream`, without launching: returns 0 (one wave per row) or 1 (the
 *   grid-stride kernel), *nv = float4 per lane of the instantiation (2, 3, 4 or 8; 8 for the direct kernel), *grid = workgroups.
 * cast_ex: out = format(in * scale_dev[0]) (scale_dev: a DEVICE float or NULL for 1); format 0: [rows, d], 1: hi|lo pair [rows, 2d] with
 *   hi = round16(v), lo = round16(v - hi), 2: mixed pair (above).  cast_to_f32: exact widening of n elements (fp32 input: a copy).
 * pack_weight: w32 [rows, cols] -> out [rows, ld_out] = round(w32) with a zero tail (ld_out >= cols), or, transposed, out [cols, ld_out]
 *   with out[c][r] = round(w32[r][c]) (ld_out >= rows; the tail is NOT written); ld_out = 0: dense; dtype fp32 / fp16 / bf16.
 * patchify: image [B, 3, R, R] of image_dtype -> out [B (R/P)^2, Kp] of dtype, out[b G^2 + gy G + gx][c P^2 + ky P + kx] =
 *   round16(image[b][c][gy P + ky][gx P + kx]), zero from column 3 P^2 on (Kp >= 3 P^2).  patchify_route: the kernel that call uses:
 *   0 scalar, 1 vector (fp32 image, P % 8 == 0), 2 the 16-byte copy (image of the compute type, P % 8 == 0, 6 P R bytes <= 64 KB). */
int mvlpt_op_layernorm_fwd_ex(int out_dtype, const float* x, int row_mul, const float* gamma, const float* beta, void* y, int rows, int d,
                              int split, mvlpt_stream_t stream);
int mvlpt_op_layernorm_bwd_ex(int dtype, const void* dy, int dy_dtype, const float* x, int row_mul, const float* gamma, const float* resid,
                              float* out32, void* out16, int rows, int d, int split, mvlpt_stream_t stream);
int mvlpt_op_layernorm_route(int rows, int d, mvlpt_stream_t stream, int* nv, int* grid);
/* The launches of the text backward under a gradient length (mvlpt_set_text_grad_len), kernel level.  A saved forward tensor holds
 * sequences of seq_pitch rows; the gradient side holds the leading grad_len rows of each, compact, and row r of it belongs to saved
 * row (r / grad_len) * seq_pitch + r % grad_len.  grad_len == seq_pitch is the plain launch.
 * gemm_gelubwd_rows: mvlpt_op_gemm_ex with epi 3 / 6 (no bias, resid, out2), `aux` [., N] read through the map; M % grad_len == 0,
 *   grad_len >= 3.  layernorm_bwd_rows: mvlpt_op_layernorm_bwd_ex with row_mul 1 and `x` alone read through the map (dy, resid, out32,
 *   out16 at row r); rows % grad_len == 0.  attention_bwd_rows: the causal attention backward over positions 0 .. grad_len-1 of N
 *   sequences: qkv / out / lse are saved tensors ([N seq_pitch, .], lse [N H seq_pitch]), dout / dqkv / delta compact
 *   ([N grad_len, .], [N H grad_len]); pair != 0: the pair kernels (mvlpt_op_attention32_bwd, lo8 != 0: _mixed; grad_len <= 80), else
 *   mvlpt_op_attention_bwd's (grad_len <= 256). */
int mvlpt_op_gemm_gelubwd_rows(int dtype, int epi, const void* A, const void* Bt, int M, int N, int K, const void* aux, void* out, int a_split,
                               int lda, int ldo, int ldb, int w8_exp, int out_lo8, int grad_len, int seq_pitch, mvlpt_stream_t stream);
int mvlpt_op_layernorm_bwd_rows(int dtype, const void* dy, int dy_dtype, const float* x, const float* gamma, const float* resid,
                                float* out32, void* out16, int rows, int d, int split, int grad_len, int seq_pitch, mvlpt_stream_t stream);
int mvlpt_op_attention_bwd_rows(int dtype, int pair, int lo8, const void* qkv, const void* out, const void* dout, const float* lse,
                                float* delta, void* dqkv, int N, int grad_len, int seq_pitch, int H, mvlpt_stream_t stream);
/* The pair attention under a shared prefix (mvlpt_set_text_shared_prefix), kernel level; causal, seq_len <= 80, lo8 != 0: mixed pairs.
 * Every tensor holds N + 1 slots: slot 0 = the prefix in its first P rows (the others are never read; the forward writes zeros into
 * them in out / lse, the backward's reduction into dqkv), slot n + 1 = positions P .. of sequence n; 2 P <= L.  fwd: qkv / out in slots of L - P rows, lse [N + 1, H, L - P].  bwd: qkv / out / lse as the forward left
 * them with L = seq_len; dout / dqkv in slots of grad_len - P rows (2 P <= grad_len); slot 0 of dout is the prefix's own dO (a class
 * sequence takes dO of its positions < P as zero).  kv_part: fp32 scratch [N + 1, P, 2 H 64].  Two launches: the backward, then the
 * reduction that writes dK / dV of slot 0 = own + part_mul * sum over the sequences, and zeros into rows P .. of slot 0. */
int mvlpt_op_attention32_fwd_prefix(int dtype, int lo8, const void* qkv, void* out, float* lse, int N, int L, int H, int prefix,
                                    mvlpt_stream_t stream);
int mvlpt_op_attention32_bwd_prefix(int dtype, int lo8, const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                                    void* dqkv, float* kv_part, float part_mul, int N, int grad_len, int seq_len, int H, int prefix,
                                    mvlpt_stream_t stream);
/* The same for single operands (the kernels of MVLPT_PREC_FAST): qkv [., 3 H 64], out / dout [., H 64], dqkv [., 3 H 64] 16-bit, slots as
 * above; delta: scratch [N + 1, H, grad_len - P]; three launches in the backward (dQ, dK / dV, the reduction). */
int mvlpt_op_attention_fwd_prefix(int dtype, const void* qkv, void* out, float* lse, int N, int L, int H, int prefix, mvlpt_stream_t stream);
int mvlpt_op_attention_bwd_prefix(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                                  float* kv_part, float part_mul, int N, int grad_len, int seq_len, int H, int prefix, mvlpt_stream_t stream);
int mvlpt_op_cast_ex(int dtype, const float* in, void* out, int64_t rows, int d, int format, const float* scale_dev, mvlpt_stream_t stream);
int mvlpt_op_cast_to_f32(int in_dtype, const void* in, float* out, int64_t n, mvlpt_stream_t stream);
int mvlpt_op_pack_weight(int dtype, const float* w32, int rows, int cols, int transposed, int ld_out, void* out, mvlpt_stream_t stream);
int mvlpt_op_patchify(int dtype, const void* image, int image_dtype, void* out, int B, int R, int P, int Kp, mvlpt_stream_t stream);
int mvlpt_op_patchify_route(int dtype, int image_dtype, int R, int P);
/* the glue of the ranged mvlpt_text_fwd / text_bwd: x [S, L, d] fp32 = assembled prompts + pos [L, d] (layout entries must address
 * rows inside prefix / suffix / ctx) and dx [S, L, d] over the sequences of HOST class_lo / class_hi int32 [G] (see MvlptTextJob;
 * lo = 0, hi = C for every g is CoCoOp's tower, S = G * C), dctx [G, n_ctx, d] = sum over group g's sequences of dx at ctx_pos
 * int32 [C, n_ctx].  These two calls wait for their kernel (test entry points). */
int mvlpt_op_assemble_prompts_ranged(const float* prefix, const float* suffix, const float* ctx, int n_ctx, const int32_t* layout,
                                     const float* pos, float* x, const int32_t* class_lo, const int32_t* class_hi, int G, int C, int L,
                                     int d, mvlpt_stream_t stream);
int mvlpt_op_gather_ctx_grad_ranged(const float* dx, const int32_t* ctx_pos, const int32_t* class_lo, const int32_t* class_hi, int G, int C,
                                    int L, int d, int n_ctx, float* dctx, mvlpt_stream_t stream);

/* ---- the dense head's neighbours and the fp32 glue of the towers at kernel level (tests/test_hip_head.py, test_hip_glue.py) ----
 * sgemm_bt: C[M,N] = alpha * A[M,K] * Bt[N,K]^T in fp32 (the two projections next to the logits and their backward); alpha_dev is a
 *   DEVICE float or NULL (1).  K % 16 == 0 and N % 4 == 0, anything else is refused.
 * grad_scale: scale_dev (3 device floats) = {2^k, 2^-k, amax|v|} with k = exponent(target) - exponent(amax) clamped to [-60, 60]
 *   (frexp exponents), 2^k = 1 when amax is 0, inf or NaN.  n <= 2^17 on a 16-byte aligned pointer runs as one workgroup, anything
 *   else as amax + finish; both give the same three floats.
 * reduce_prompt_rows: out [n,d] = scale_dev[1] (or 1 when NULL) * sum_b dx32[b, row0 + j, :] (* vmask [B,n,d] when given) over
 *   dx32 [B,L,d]; zero_after != 0 clears those rows of dx32 and of its 16-bit copy dx16 (may be NULL; split16 0: [B*L, d], 1: hi|lo pair
 *   [B*L, 2d], 2: mixed pair at the same pitch) afterwards.  d % 4 == 0.
 * gather_ctx_grad: dctx [n_ctx,d] = scale_dev[1] * sum_c dx[c, ctx_pos[c,j], :] (per_class = 0) or dctx [C,n_ctx,d] without the sum
 *   (per_class = 1); dx [C,L,d], ctx_pos int32 [C,n_ctx] with entries in [0, L).
 * attention_bwd_cls: the attention backward when only query 0 of every sequence carries a gradient: qkv [N*L, 3*H*64] 16-bit,
 *   o_cls / do_cls [N, H*64] (row 0 of every sequence), lse [N*H*L] -> dqkv [N*L, 3*H*64], every element written (dQ rows > 0 are 0).
 * copy_rows: dst[r] = src[idx[r]] (scatter = 0) or dst[idx[r]] = src[r] (scatter = 1) for `rows` rows of row_bytes (% 16 == 0).
 * overwrite_rows: x[b, 1 + j, :] = rows[j, :] (* vmask[b, j, :]) for j < n, x [B,L,d] fp32.
 * assemble_tokens: the image tower's entry, x [B, 1 + n_vpt + G2, d]: row 0 = LN(cls + pos[0]), rows 1..n_vpt = vpt (* vmask [B,n_vpt,d]),
 *   the rest LN(patch_emb[b, i] + pos[1 + i]); pos [1 + G2, d].
 * assemble_prompts: the text tower's entry (arguments of mvlpt_text_fwd): x [C,L,d] = prompts + pos, eot_rows int32 [C] = c * L + eot[c],
 *   and, when n_ctx > 0, ctx_pos int32 [C,n_ctx] = position of context row j in class c's sequence. */
/* ---- the zero-shot glue at kernel level (tests/test_hip_zsclip_ops.py) ----
 * embed_tokens: x [S, L, d] = emb[ids[s, t]] + pos[t] with ids a DEVICE int32 [S, ld] table, ld >= L, columns 0 .. L-1 read; the caller
 *   guarantees those ids are rows of emb.  d % 4 == 0.
 * ensemble_features: the kernel of mvlpt_text_ensemble.  normalize_rows: xn = x / |x|, norm = |x| per row (the head's normalisation). */
int mvlpt_op_embed_tokens(const float* emb, const float* pos, const int32_t* ids, int ld, float* x, int S, int L, int d,
                          mvlpt_stream_t stream);
int mvlpt_op_ensemble_features(const float* feats, float* out, int T, int C, int e, mvlpt_stream_t stream);
int mvlpt_op_normalize_rows(const float* x, float* xn, float* norm, int rows, int d, mvlpt_stream_t stream);
int mvlpt_op_sgemm_bt(const float* A, const float* Bt, float* C, int M, int N, int K, const float* alpha_dev, mvlpt_stream_t stream);
int mvlpt_op_grad_scale(const float* v, int64_t n, float target, float* scale_dev, mvlpt_stream_t stream);
int mvlpt_op_reduce_prompt_rows(int dtype, float* dx32, void* dx16, int B, int L, int d, int row0, int n, float* out,
                                const float* scale_dev, int zero_after, int split16, const float* vmask, mvlpt_stream_t stream);
int mvlpt_op_gather_ctx_grad(const float* dx, const int32_t* ctx_pos, int C, int L, int d, int n_ctx, int per_class, float* dctx,
                             const float* scale_dev, mvlpt_stream_t stream);
int mvlpt_op_attention_bwd_cls(int dtype, const void* qkv, const void* o_cls, const void* do_cls, const float* lse, void* dqkv, int N,
                               int L, int H, mvlpt_stream_t stream);
int mvlpt_op_copy_rows(const void* src, void* dst, const int32_t* idx, int rows, int row_bytes, int scatter, mvlpt_stream_t stream);
int mvlpt_op_overwrite_rows(const float* rows, int n, float* x, int B, int L, int d, const float* vmask, mvlpt_stream_t stream);
/* the glue of the deep mvlpt_text_fwd / text_bwd (tests/test_hip_deep_text_ops.py); ctx_pos int32 [C,n_ctx] with entries in [0, L)
 * (an entry outside is skipped), d % 4 == 0:
 * overwrite_ctx_rows: x[c, ctx_pos[c,j], :] = rows[j, :], x [C,L,d] fp32, rows [n_ctx,d]; no other row is written.
 * gather_zero_ctx_grad: out [n_ctx,d] = scale_dev[1] (or 1 when NULL) * sum_c dx32[c, ctx_pos[c,j], :] with the bits of
 *   gather_ctx_grad (per_class = 0), then those rows of dx32 [C,L,d] and of its 16-bit copy dx16 (may be NULL; split16 as in
 *   reduce_prompt_rows; of a mixed row the hi plane and the d residual bytes) are zero; nothing else is written. */
int mvlpt_op_overwrite_ctx_rows(const float* rows, const int32_t* ctx_pos, float* x, int C, int L, int d, int n_ctx, mvlpt_stream_t stream);
int mvlpt_op_gather_zero_ctx_grad(int dtype, float* dx32, void* dx16, int split16, const int32_t* ctx_pos, int C, int L, int d, int n_ctx,
                                  float* out, const float* scale_dev, mvlpt_stream_t stream);
int mvlpt_op_assemble_tokens(const float* patch_emb, const float* cls, const float* pos, const float* ln_g, const float* ln_b,
                             const float* vpt, int n_vpt, const float* vmask, float* x, int B, int G2, int d, mvlpt_stream_t stream);
int mvlpt_op_assemble_prompts(const float* prefix, const float* suffix, const float* ctx, int ctx_per_class, int n_ctx,
                              const int32_t* layout, const float* pos, const int32_t* eot, float* x, int32_t* ctx_pos, int32_t* eot_rows,
                              int C, int L, int d, mvlpt_stream_t stream);

/* ---- the convolutional tower at kernel level (tests/test_hip_conv.py).  fp16 NHWC activations; handle-free, enqueue-only; every
 * argument error (a NULL pointer, an extent <= 0, a shape outside the limits) returns MVLPT_ERR_ARG or MVLPT_ERR_UNSUPPORTED with a
 * message in mvlpt_last_error(NULL) before anything is launched.
 * pack_conv_weight: w32 [Cout, Cin, k, k] fp32 -> out fp16 [Cout, Kp], column (ky * k + kx) * cin_pad + ci (tap-major: a tap's channel
 *   run is contiguous, as in the NHWC input), zero for ci >= Cin and for the tail; Kp = k * k * cin_pad rounded up to 32 is returned
 *   through *kp (out may be NULL to ask for it).  cin_pad >= Cin, cin_pad % 8 == 0.
 * conv2d: y [B, Ho, Wo, Cout] = act(conv(x [B, H, W, Cin], w) * scale[c] + shift[c] (+ resid [B, Ho, Wo, Cout])), act = ReLU when
 *   relu != 0; fp32 accumulation and epilogue, ONE rounding to fp16.  k in {1, 3}, pad k / 2, stride 1, or 2 with k = 3;
 *   Ho = (H + 2 pad - k) / stride + 1; Cin (= the weight's cin_pad) % 8 == 0, Cout % 8 == 0 (MVLPT_ERR_UNSUPPORTED otherwise);
 *   scale / shift fp32 [Cout].  Out-of-image taps are zero; pointers 16-byte aligned.
 * avgpool2x2: AvgPool2d(2), y [B, H/2, W/2, C], fp32 sum of four and one rounding; C % 8 == 0.
 * nchw_to_nhwc8: image [B, 3, R, R] of image_dtype (MVLPT_DT_*) -> [B, R, R, 8] fp16, channels 3..7 zero.
 * attnpool_tokens: tok [B, 1 + HW, E] fp16 = [mean over HW ; x [B, HW, E]] + pos [1 + HW, E] fp32 (mean and sum in fp32, one rounding).
 * attnpool_query: out [B, E] fp16: per image and head of 64 channels softmax(q . K / 8) V with q [B, E], kv [B, T, 2E] = [K | V];
 *   scores and softmax in fp32; 1 <= T <= 145, E % 64 == 0. */
int mvlpt_op_pack_conv_weight(const float* w32, int Cout, int Cin, int k, int cin_pad, void* out, int* kp, mvlpt_stream_t stream);
int mvlpt_op_conv2d(const void* x, const void* w, const float* scale, const float* shift, const void* resid, void* y, int B, int H,
                    int W, int Cin, int Cout, int k, int stride, int relu, mvlpt_stream_t stream);
int mvlpt_op_avgpool2x2(const void* x, void* y, int B, int H, int W, int C, mvlpt_stream_t stream);
int mvlpt_op_nchw_to_nhwc8(const void* image, int image_dtype, void* out, int B, int R, mvlpt_stream_t stream);
int mvlpt_op_attnpool_tokens(const void* x, const float* pos, void* tok, int B, int HW, int E, mvlpt_stream_t stream);
int mvlpt_op_attnpool_query(const void* q, const void* kv, void* out, int B, int T, int E, mvlpt_stream_t stream);

/* ---- fused optimizer step over the flat prompt buffers (row f2 of the scope table; tests/test_hip_optim.py) ----
 * ONE launch updates param, state1 and state2 in place over [0, n) with torch.optim's single-tensor formulas in fp32:
 *   SGD   (kind 0): d = g + wd p;  buf = d on a segment's first step, else m buf + (1 - damp) d;  p -= lr (nesterov ? d + m buf : buf);
 *                   momentum == 0: no buffer (state1 may be NULL), p -= lr d.
 *   Adam  (kind 1): g' = g + wd p;                      AdamW (kind 2): p *= 1 - lr wd, g' = g;   then, with t the segment's step count,
 *                   m += (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps).
 * The buffers are the parameter tensors back to back, 16-byte aligned; segs_dev (DEVICE, n_segs <= MVLPT_OPTIM_MAX_SEGS entries sorted by
 * `begin`, not overlapping, boundaries arbitrary) names them.  A segment with active == 0 (a parameter without a gradient), and any
 * element no segment covers, is not touched, bit for bit.  A segment's step count is t = launch - missed: the caller adds to `missed`
 * the launches a segment sat out when it comes back, so a table whose active set does not change is never uploaded again.
 * `hyper` is HOST memory, read at call time.  loss_dev (DEVICE float, or NULL): when *loss_dev is NaN or +-inf the launch writes
 * nothing to param / state1 / state2 and adds 1 to *skipped_dev (DEVICE int32, or NULL), once per launch.  Enqueue-only on `stream`. */
enum { MVLPT_OPTIM_SGD = 0, MVLPT_OPTIM_ADAM = 1, MVLPT_OPTIM_ADAMW = 2 };
enum { MVLPT_OPTIM_MAX_SEGS = 1024 };
typedef struct MvlptOptimSeg {
  int64_t begin, end;             /* elements [begin, end) of the flat buffers */
  int32_t active;                 /* 0: the parameter has no gradient this step */
  int32_t missed;                 /* launches this segment did not take part in */
} MvlptOptimSeg;
typedef struct MvlptOptimHyper {
  int32_t kind;                   /* MVLPT_OPTIM_* */
  int32_t nesterov;
  /* doubles, as torch.optim holds them: the kernel's fp32 constants (1 - beta, 1 - dampening, 1 - lr wd, the bias corrections) are
   * formed in double and rounded once — 1 - beta2^t from a beta2 already rounded to fp32 would be off by 1e-5 of its value */
  double lr, weight_decay, momentum, dampening;
  double beta1, beta2, eps;
  int64_t launch;                 /* 1-based count of step calls */
} MvlptOptimHyper;
int mvlpt_op_optim_step(const MvlptOptimHyper* hyper, float* param, const float* grad, float* state1, float* state2, int64_t n,
                        const MvlptOptimSeg* segs_dev, int n_segs, const float* loss_dev, int32_t* skipped_dev, mvlpt_stream_t stream);

/* ---- prompt interpretation: the nearest vocabulary tokens of context vectors (row i of the scope table; tests/test_hip_nearest.py) ----
 * Replaces `torch.cdist(ctx, token_embedding)` + `torch.argsort(distance, dim=1)[:, :topk]` (scripts/interpret_prompt.py:49-59) with a
 * fused distance + top-k: for every row of q [R, d] fp32 the k rows of table [V, d] fp32 (row-major) with the smallest Euclidean
 * distance, ascending, into idx int32 [R, k] and dist fp32 [R, k].  No [R, V] array exists at any point; the scratch memory is partial
 * lists of k (distance, index) pairs per row, mvlpt_nearest_workspace_bytes of them.
 *   Distance: s = sum_i (q_i - e_i)^2 in the difference form (never |q|^2 + |e|^2 - 2 q.e, which cancels), fp32, the d terms of a
 *     (row, token) pair added in the order i = 0 .. d-1 whatever the pair's place in the table, the row tile, the vocabulary slice or
 *     the grid; dist = sqrtf(s), correctly rounded.  So |dist - exact| <= (d / 2 + 3) * 2^-24 * exact, a query that is a copy of a
 *     table row is at distance exactly 0.0, bitwise copies of a table row tie exactly, and the results do not depend on the stream's
 *     compute units (mvlpt_stream_create_cus, mvlpt_stream_set_cu_cap) or on a rerun.
 *   Order: the key is (s, token index): smaller s first, equal s by smaller index (torch.argsort leaves ties open).  A NaN s orders
 *     behind every number, +inf included, as torch.sort places it; NaNs among themselves by index.  A query row of NaN or of +-inf
 *     therefore returns tokens 0 .. k-1 with NaN / +inf distances, and a table row that holds a NaN is returned only when fewer than
 *     k other rows exist.  The selection is exact on this order: nothing is sampled or approximated.
 *   Limits: R >= 1, V >= 1, 1 <= k <= min(V, MVLPT_NEAREST_MAX_K), d % 4 == 0, 4 <= d <= 1024, R <= MVLPT_NEAREST_MAX_ROWS (the row
 *     tile rides on grid.y; callers chunk R), q / table 16-byte aligned.  Every violation, a NULL pointer and a workspace below
 *     mvlpt_nearest_workspace_bytes return MVLPT_ERR_ARG (k > MVLPT_NEAREST_MAX_K: MVLPT_ERR_UNSUPPORTED) before anything is launched;
 *     the outputs are not touched.
 * mvlpt_nearest_workspace_bytes: *out = bytes mvlpt_op_nearest_rows needs for these sizes on `stream` (the number of vocabulary
 *   slices follows mvlpt_stream_cus(stream) so that R = 16 still fills the device: ask again after the stream's cap has changed).
 * mvlpt_op_nearest_rows: the kernel-level entry, handle-free (errors: mvlpt_last_error(NULL)); the caller owns `workspace`;
 *   enqueue-only on `stream`.
 * mvlpt_nearest_tokens: the same against the engine's resident "token_embedding.weight" (d = text_width, V = vocab), scratch from the
 *   engine's grow-only workspace; MVLPT_ERR_STATE when the table has not been passed to mvlpt_load_frozen. */
enum { MVLPT_NEAREST_MAX_K = 64 };
enum { MVLPT_NEAREST_MAX_ROWS = 65535 * 8 };
int mvlpt_nearest_workspace_bytes(int R, int V, int d, int k, mvlpt_stream_t stream, int64_t* out);
int mvlpt_op_nearest_rows(const float* q, const float* table, int R, int V, int d, int k, int32_t* idx, float* dist, void* workspace,
                          int64_t workspace_bytes, mvlpt_stream_t stream);
int mvlpt_nearest_tokens(void* handle, const float* q, int R, int k, int32_t* idx, float* dist, mvlpt_stream_t stream);

/* ---- test-time prompt tuning: the entropy head over V views per image (row o of the scope table; tests/test_hip_tpt_head.py) ----
 * Replaces, per optimisation step of TPT (Shu et al., NeurIPS 2022), the logits product, log_softmax, per-view entropy, the
 * argsort-based confidence selection, the marginal entropy of the selected views and autograd back to the text features.
 * All fp32, row-major: img [G, V, e] un-normalised features of the V views of each of G test images; txt [G*C, e] un-normalised text
 * features, row g*C + c = (image g, class c) (a ranged mvlpt_text_fwd over full ranges); scale = exp(logit_scale); 1 <= k <= V.
 *   Forward:  z[g,v,c] = scale <img/|img|, txt/|txt|>;  logp = z - logsumexp_c z;  H[g,v] = -sum_c exp(logp) logp;
 *     sel[g] = the k views with the smallest H under the total order (H, then view index), NaN behind every number, written as
 *     int32 [G, k] in that order;  a[g,c] = logsumexp_{v in sel[g]} logp[g,v,c] - log k;  loss[g] = -sum_c exp(a) a.
 *     Outputs loss [G], H [G, V], sel [G, k]; z [G, V, C] only when the pointer is not NULL (tests): no [G, V, C] array is written
 *     otherwise.  C = 1 gives H = 0 and loss = 0 exactly.
 *   Backward: d (sum_g w_g loss[g]) / d txt with the selection held constant (w [G] on the device, NULL: all 1):
 *     p = exp(logp), u_c = -(a_c + 1), dz[g,v,j] = (w_g / k) p_vj (u_j - sum_c p_vc u_c) for v in sel[g], 0 otherwise;
 *     dtn[g,c] = scale sum_{v in sel} dz[g,v,c] img_v/|img_v|;  dtxt[g*C+c] = (dtn - <dtn, tn> tn) / |txt|.  Output dtxt [G*C, e];
 *     there is no dimg (the image tower is frozen on this route).
 *     The backward READS the workspace its forward filled (normalised rows, |txt|, the selection, logp and a of the selected views)
 *     and recomputes nothing: it must follow mvlpt_op_tpt_head_fwd with the same sizes on the same stream and workspace, with nothing
 *     else written to the workspace in between; it may be repeated (other weights).  It does not read img / txt / sel again.
 *   Arithmetic: fp32 vector ALU; one lane adds the e terms of a (view, class) pair in the order i = 0 .. e-1, so the bits of z and of
 *     H depend on the view's and the group's rows alone: not on the view's position v, the group's index, G or a rerun.  Two
 *     bit-identical views have bit-identical H and resolve by index.  No floating-point atomics; every sum has one order.
 *   Limits: 1 <= G <= MVLPT_TPT_MAX_GROUPS, 1 <= V <= MVLPT_TPT_MAX_VIEWS, 1 <= C <= MVLPT_TPT_MAX_CLASSES, G * C < 2^31,
 *     4 <= e <= 1024 with e % 4 == 0, 1 <= k <= V; img, txt, dtxt and the workspace 16-byte aligned.  Every violation, a NULL required
 *     pointer and a workspace below mvlpt_tpt_workspace_bytes return MVLPT_ERR_ARG (message: mvlpt_last_error(NULL)) before anything
 *     is launched; nothing is written.  Handle-free, enqueue-only on `stream`, offsets are 64-bit. */
enum { MVLPT_TPT_MAX_VIEWS = 128 };
enum { MVLPT_TPT_MAX_GROUPS = 65535 };
enum { MVLPT_TPT_MAX_CLASSES = 1 << 20 };
int mvlpt_tpt_workspace_bytes(int G, int V, int C, int e, int k, int64_t* bytes);
int mvlpt_op_tpt_head_fwd(const float* img, const float* txt, float scale, int G, int V, int C, int e, int k, float* loss, float* H,
                          int32_t* sel, float* z, void* workspace, int64_t workspace_bytes, mvlpt_stream_t stream);
int mvlpt_op_tpt_head_bwd(const float* w, float scale, int G, int V, int C, int e, int k, float* dtxt, void* workspace,
                          int64_t workspace_bytes, mvlpt_stream_t stream);

/* ---- evaluation on the device: class counters and column rank statistics (row f1b of the scope table; tests/test_hip_eval.py) ----
 * Everything MVLPT.test reports is a function of integer counts; these two entries produce the counts exactly, and the few remaining
 * double-precision divisions and means are finished on the host (mvlpt_amd/evaluator.py) with the calls mvlpt_amd/metrics.py makes.
 * Both are handle-free (errors: mvlpt_last_error(NULL)) and enqueue-only on `stream`; a NULL required pointer, an extent outside its
 * limits, a pitch below the width or a workspace that is too small return MVLPT_ERR_ARG (N > MVLPT_EVAL_MAX_ROWS:
 * MVLPT_ERR_UNSUPPORTED) before anything is launched.  Device index arrays are the caller's responsibility: a row index, task id or
 * int64 label outside its extent is clamped or skipped (nothing is read or written out of bounds; the counts are then meaningless).
 *
 * mvlpt_op_eval_count: streaming class counters, one launch per evaluation batch and no host sync.  Replaces the per-batch
 *   `output.max(1)[1]`, the Python loop over `set(tasks_)` with its boolean masks and ranged arg-max (trainers/mvlpt.py:1023-1045) and
 *   the arg-max of balanced_accuracy_score (trainers/vision_benchmark/datasets/metrics.py:1271-1274 behind filter_out_zero_tgt).
 *   logits fp32 [B, C] with row pitch ld >= C.  labels: int64 [B] (MVLPT_LABEL_INT64) or fp32 [B, C] with pitch label_ld
 *   (MVLPT_LABEL_PROB_F32: the row's arg-max is its label, as `label.argmax(dim=1)`).  rows: optional int32 [n_rows] list of the rows
 *   that are counted (NULL: all B rows).  task int32 [B] with lo / hi int32 [T] (device; all three or none): the row's own class range.
 *   col_mask: optional uint8 [C]; every arg-max, the label's included, then runs over the columns with a non-zero byte only.
 *   col_seen: optional uint8 [C] output, set to 1 for every column that holds a non-zero target (the int64 label's column) in a counted
 *   row and otherwise left alone: the column-occurrence pass whose result is the col_mask of mean-per-class (filter_out_zero_tgt).
 *   Added into caller-owned int64 device buffers: n_true[C], n_pred[C], n_hit[C] for the arg-max over all columns; with ranges
 *   n_pred_r[C], n_hit_r[C] for the arg-max over [lo_t, hi_t); cmat (optional) [C, C] indexed (true, pred).  Arg-max as numpy: the
 *   lowest index among equal maxima, a NaN counts as maximal.  The adds are 64-bit integer atomics: the result does not depend on the
 *   order of the rows or on a rerun.  No floating-point atomics.
 *
 * mvlpt_op_eval_rank_columns: per column c of scores fp32 [N, C] (pitch ld >= C: a column slice is read in place), over the rows of
 *   the optional int32 list `rows` [n_rows] (NULL: all N rows; a non-NULL list may be empty, n_rows <= N), with a target that is
 *   positive where int64 labels[row] == c (MVLPT_LABEL_INT64) or where the fp32 matrix [N, target_ld] holds exactly 1
 *   (MVLPT_LABEL_PROB_F32), the sorted-order statistics that roc_auc_score and the 11-point walk of map_11_points read
 *   (metrics.py:1265-1268, 1277-1280, 853-895).  Scores order by value, -0.0 and +0.0 are one value:
 *     n_pos[c], n_neg[c]   int64
 *     twice_u[c]           int64: sum over the runs [a, b) of equal scores in ascending order of (positives in the run) * (a + 1 + b),
 *                          minus n_pos * (n_pos + 1): twice the tie-averaged Mann-Whitney U
 *     interp[c * 11 + i]   double: the largest precision tp / cnt among the points (one per run start a: tp = positives at or behind a,
 *                          cnt = n - a, recall = tp / n_pos, or 1 when n_pos == 0; plus the closing point precision 1, recall 0) with
 *                          thresholds[i] <= recall, 0 when there is none.  thresholds: 11 HOST doubles.  IEEE double divisions.
 *     flags[c]             int32: MVLPT_EVAL_FLAG_NONFINITE when a selected score of the column is NaN or +-inf (numpy's np.diff splits
 *                          runs of equal infinities; the caller then finishes that metric on the host);
 *                          MVLPT_EVAL_FLAG_SOFT_TARGET when a selected fp32 target of the column is neither 0 nor 1 (metrics.py keeps a
 *                          column for any non-zero target but counts only 1 as positive: the host decides such inputs too).
 *   One workgroup sorts one column: in LDS up to MVLPT_EVAL_SORT_TILE rows, beyond that with `workspace` for the long strides.
 * mvlpt_eval_workspace_bytes: *out = bytes mvlpt_op_eval_rank_columns needs for at most N selected rows and C columns on `stream`
 *   (0 when the columns fit in LDS: the workspace may then be NULL). */
enum { MVLPT_EVAL_SORT_TILE = 4096 };
enum { MVLPT_EVAL_MAX_ROWS = 1 << 20 };
enum { MVLPT_EVAL_POINTS = 11 };
enum { MVLPT_EVAL_FLAG_NONFINITE = 1, MVLPT_EVAL_FLAG_SOFT_TARGET = 2 };
int mvlpt_op_eval_count(const float* logits, int64_t ld, int B, int C, const void* labels, int label_kind, int64_t label_ld,
                        const int32_t* rows, int n_rows, const int32_t* task, const int32_t* lo, const int32_t* hi, int T,
                        const uint8_t* col_mask, uint8_t* col_seen, int64_t* n_true, int64_t* n_pred, int64_t* n_hit, int64_t* n_pred_r,
                        int64_t* n_hit_r, int64_t* cmat, mvlpt_stream_t stream);
int mvlpt_op_eval_rank_columns(const float* scores, int64_t ld, int N, int C, const void* targets, int target_kind, int64_t target_ld,
                               const int32_t* rows, int n_rows, const double* thresholds, int64_t* n_pos, int64_t* n_neg,
                               int64_t* twice_u, double* interp, int32_t* flags, void* workspace, int64_t workspace_bytes,
                               mvlpt_stream_t stream);
int mvlpt_eval_workspace_bytes(int N, int C, mvlpt_stream_t stream, int64_t* out);

/* ---- linear-probe CLIP baseline: L2-regularised multinomial logistic regression (row j of the scope table; tests/test_hip_softmax_reg.py) ----
 * Replaces sklearn's LogisticRegression(solver="lbfgs", penalty="l2", C=C) of lpclip/linear_probe.py with full-batch evaluations on
 * the device.  The objective is the one sklearn 1.7 minimises,
 *     F(W, b) = (1/N) sum_i [logsumexp(z_i) - z_i[y_i]] + (l2/2) |W|_F^2,   z_i = W x_i + b,   l2 = 1 / (C N),   b unpenalised.
 * theta = [W row-major [K, D] | b [K]] fp32; grad has the same layout; X [N, D] fp32 row-major; y int32 [N] on the DEVICE, every
 * label in [0, K) (the caller's responsibility at this level: a label outside matches no class, nothing is read out of bounds).
 *   mvlpt_op_softmax_reg_eval: grad = dF/dtheta and stats = {F, max|grad|, grad . dir (0 when dir is NULL), |grad|^2}, four doubles on
 *     the device.  The logits are an fp32 product on the fp32-input matrix instruction; max, log-sum-exp, loss and the probabilities
 *     are formed in double from them; R = (p - onehot) / N is rounded once to fp32; grad_W = R^T X over row slices whose count depends
 *     on (N, D, K) alone, the slices added in double in slice order with l2 W and rounded once; grad_b = the column sums of R in
 *     double; the statistics in double.  No floating-point atomics: the bits of every output depend on the inputs and the shape alone.
 *   mvlpt_op_softmax_reg_predict: pred[i] = arg max_k z_i[k], the lowest class index among equal logits (numpy's rule), and, when
 *     margin is not NULL, margin[i] = largest - second largest logit (0 for a tie).  Callers chunk the rows to bound the workspace.
 *   mvlpt_softmax_reg_workspace_bytes: the bytes either entry needs for these sizes (predict uses the first N * roundup(K, 4) floats).
 *   Limits: N >= 1, K >= 2, D >= 4, D % 4 == 0, K * (D + 1) < 2^31; X, theta and the workspace 16-byte aligned.  Every violation, a
 *     NULL pointer and a workspace that is too small return MVLPT_ERR_ARG with a message (mvlpt_last_error(NULL)) before anything is
 *     launched.  Handle-free and enqueue-only on `stream`; offsets are 64-bit. */
int mvlpt_softmax_reg_workspace_bytes(int N, int D, int K, size_t* bytes);
int mvlpt_op_softmax_reg_eval(const float* X, const int32_t* y, const float* theta, const float* dir, int N, int D, int K, double l2,
                              float* grad, double* stats, void* ws, size_t ws_bytes, mvlpt_stream_t stream);
int mvlpt_op_softmax_reg_predict(const float* X, const float* theta, int N, int D, int K, int32_t* pred, float* margin, void* ws,
                                 size_t ws_bytes, mvlpt_stream_t stream);

/* ---- Tip-Adapter / Tip-Adapter-F: the fused key-value cache head (row p of the scope table; tests/test_hip_tip.py) ----
 * Replaces, per call of Tip-Adapter (Zhang et al., ECCV 2022), `exp(-beta (1 - F K^T)) @ one_hot`, its [N, NK] array and the sum with
 * the zero-shot logits; for Tip-Adapter-F the cross-entropy and autograd back to the keys; for the hyper-parameter search the loop over
 * the (beta, alpha) grid.  All fp32, row-major: F [N, D] unit image features, K [NK, D] the cache keys SORTED BY CLASS, key_ptr int32
 * [C + 1] on the device (non-decreasing, key_ptr[0] = 0, key_ptr[C] = NK: class c owns the keys [key_ptr[c], key_ptr[c + 1])), W [C, D]
 * unit text features, s = exp(logit_scale).  A class may own no key: its cache term is exactly alpha * 0.
 *     z[n, c] = s <f_n, w_c> + alpha * sum_{j in c} A[n, j],   A[n, j] = exp(beta * (<f_n, k_j> - 1)).
 *   mvlpt_op_tip_logits: logits [N, C] = z.  No [N, NK] array exists.
 *   mvlpt_op_tip_train_fwd: with labels y int32 [N] on the device, each in [0, C): loss [1] = the mean cross-entropy of z, correct [1]
 *     (int32) = the rows whose arg-max is y; logits [N, C] only when the pointer is not NULL.  The workspace keeps A [N, NK] and
 *     r = (softmax(z) - onehot) / N for the backward.  The row statistics are formed in double from the fp32 logits, the loss partials
 *     added in double in a fixed order.  C = 1 gives loss = 0 and r = 0 exactly.
 *   mvlpt_op_tip_train_bwd: dK [NK, D] = alpha beta sum_n A[n, j] r[n, cls(j)] f_n; the factor A r is formed while the operand is staged,
 *     no [N, NK] gradient array is written.  Only the keys carry a gradient.  It READS the workspace of its forward: same sizes, stream
 *     and workspace, nothing else written to the workspace in between; it may be repeated.  alpha = 0 or beta = 0 gives dK = 0.
 *   mvlpt_op_tip_search: betas [nb], alphas [na] on the device; counts int32 [nb, na] = the rows whose arg-max of z at (betas[b],
 *     alphas[a]) is y.  The affinity product is formed once, not per grid point; one exponential per (affinity, beta); alpha enters in
 *     the arg-max alone.  The workspace holds one row chunk of [C, nb + 1] floats per row (about 512 MiB at most, or one block of 128
 *     rows); the chunks follow each other on the stream.  The logits of a grid point have the bits mvlpt_op_tip_logits gives there.
 *   mvlpt_tip_workspace_bytes: the bytes an entry needs; mode MVLPT_TIP_LOGITS (0: nb and na ignored), MVLPT_TIP_TRAIN (nb and na
 *     ignored) or MVLPT_TIP_SEARCH.
 *   Arithmetic: products on the fp32-input matrix instruction.  The keys of a class are added one by one in ascending order; every sum
 *     has an order fixed by the sizes and key_ptr alone, so two calls are bit-equal and a row's logits do not depend on the rows
 *     around it.  Arg-max ties go to the lowest class.  No
 *     floating-point atomics; the search counts are integer atomic adds.
 *   Limits: 1 <= N, NK <= MVLPT_TIP_MAX_ROWS, 1 <= C <= MVLPT_TIP_MAX_CLASSES, D >= 4 with D % 4 == 0, N * C < 2^31, 1 <= nb <= MVLPT_TIP_MAX_NB,
 *     1 <= na <= MVLPT_TIP_MAX_NA; F, K, W, dK and the workspace 16-byte aligned.  Every violation, a NULL required pointer and a
 *     workspace below mvlpt_tip_workspace_bytes return MVLPT_ERR_ARG (message: mvlpt_last_error(NULL)) before anything is launched;
 *     nothing is written.  key_ptr and y are trusted: the caller validates them on the host.  Handle-free, enqueue-only on `stream`. */
enum { MVLPT_TIP_LOGITS = 0, MVLPT_TIP_TRAIN = 1, MVLPT_TIP_SEARCH = 2 };
enum { MVLPT_TIP_MAX_NB = 256, MVLPT_TIP_MAX_NA = 32 };
enum { MVLPT_TIP_MAX_CLASSES = 1 << 20 };
enum { MVLPT_TIP_MAX_ROWS = 2147483392 };      /* 2^31 - 256: row and key counts are rounded up to whole tiles in 32 bits */
int mvlpt_tip_workspace_bytes(int N, int NK, int C, int D, int nb, int na, int mode, int64_t* bytes);
int mvlpt_op_tip_logits(const float* F, const float* K, const int32_t* key_ptr, const float* W, float s, float alpha, float beta, int N,
                        int NK, int C, int D, float* logits, mvlpt_stream_t stream);
int mvlpt_op_tip_train_fwd(const float* F, const int32_t* y, const float* K, const int32_t* key_ptr, const float* W, float s, float alpha,
                           float beta, int N, int NK, int C, int D, float* loss, int32_t* correct, float* logits, void* workspace,
                           int64_t workspace_bytes, mvlpt_stream_t stream);
int mvlpt_op_tip_train_bwd(const float* F, float alpha, float beta, int N, int NK, int C, int D, float* dK, void* workspace,
                           int64_t workspace_bytes, mvlpt_stream_t stream);
int mvlpt_op_tip_search(const float* F, const int32_t* y, const float* K, const int32_t* key_ptr, const float* W, float s,
                        const float* betas, const float* alphas, int N, int NK, int C, int D, int nb, int na, int32_t* counts,
                        void* workspace, int64_t workspace_bytes, mvlpt_stream_t stream);

/* ---- input pipeline ("next" row f3 of the scope table) -------------------------------------------------------
 * Replaces the per-image CPU transform the reference runs in DataLoader workers: Dassl `build_transform` with
 * INPUT.TRANSFORMS = random_resized_crop / random_flip / normalize, INTERPOLATION bicubic, CLIP PIXEL_MEAN/STD
 * (configs/trainers/MVLPT/vit_b16.yaml:8-13), and the ELEVATER eval transform Resize(BICUBIC) [+ CenterCrop] +
 * ToTensor + Normalize (trainers/vision_benchmark/evaluation/feature.py:538-553).  Both are torchvision ops on PIL
 * images: `img.crop(box).resize((rw, rh), BICUBIC)` [+ window] [+ horizontal flip], u8/255, (x - mean)/std.
 * The random parameters (crop box, flip) are drawn by the caller (host RNG, as torchvision does).
 * Results are bit-identical to Pillow (8-bit resample) and torch CPU (fp32 arithmetic). */
typedef struct MvlptImageDesc {
  int64_t offset;                 /* byte offset of pixel (0,0) in `src`; image = uint8 HWC, 3 channels, row stride 3*width */
  int32_t height, width;
  int32_t crop_top, crop_left, crop_height, crop_width;   /* PIL crop box, inside the image */
  int32_t resize_height, resize_width;                    /* size the crop is resampled to */
  int32_t out_top, out_left;                              /* window [out_top, out_top+out_h) x [out_left, out_left+out_w)
                                                             of the resized image that is produced (CenterCrop); 0, 0 if none */
  int32_t flip;                                           /* 1 = horizontal flip of the produced window */
  int32_t reserved;
} MvlptImageDesc;
/* src: device, packed decoded images; descs: HOST array of B descriptors (uploaded on `stream`);
 * out: device [B,3,out_h,out_w] of out_dtype (MVLPT_DT_*), may be NULL; out_u8: device [B,out_h,out_w,3] resized 8-bit
 * image before ToTensor (may be NULL; parity tests).  mean/std: 3 host floats each. */
int mvlpt_preprocess(void* handle, const uint8_t* src, int64_t src_bytes, const MvlptImageDesc* descs, int B, int out_h, int out_w,
                     const float* mean, const float* std, void* out, int out_dtype, uint8_t* out_u8, mvlpt_stream_t stream);

/* ---- augmented input pipeline (row f3b of the scope table) ---------------------------------------------------
 * The augmentations of Dassl's `build_transform` beyond those three (the launcher's --transforms): colorjitter,
 * randomgrayscale, random_crop with zero padding, cutout.  torchvision runs them on PIL images: ColorJitter is
 * `ImageEnhance.Brightness / Contrast / Color` and an HSV round trip in a drawn order, RandomGrayscale is `convert("L")`,
 * RandomCrop(padding) is `pad(fill=0)` in front of a crop, and Dassl's Cutout zeroes rectangles of the tensor before
 * Normalize.  The caller draws the parameters; the pixels are bit-identical to Pillow's and torch's:
 *   L                (R*19595 + G*38470 + B*7471 + 0x8000) >> 16
 *   blend(d, x, a)   t = (float)d + a * (float)(x - d) in fp32; 0 <= a <= 1: (uint8)(int)t; else t <= 0 -> 0, t >= 255 -> 255, else (int)t
 *   brightness       blend(0, x, factor[0]);  saturation: blend(L of the pixel, x, factor[2])
 *   contrast         blend(m, x, factor[1]), m = (int)((double)(sum of L) / (double)(out_h*out_w) + 0.5) over the whole output
 *                    window, padding included, of the image as it stands at that point of the chain
 *   hue              Pillow's RGB -> HSV, H = (H + hue_shift) & 255, HSV -> RGB; it runs for a shift of 0 too and is not the identity
 *   grayscale        every channel := L;  holes: the rectangle := 0 in all channels
 * Order per image: resample -> window -> flip -> ops[0..n_ops) -> grayscale -> holes -> ToTensor -> Normalize. */
#define MVLPT_AUG_MAX_HOLES 4
#define MVLPT_AUG_BRIGHTNESS 0
#define MVLPT_AUG_CONTRAST 1
#define MVLPT_AUG_SATURATION 2
#define MVLPT_AUG_HUE 3
typedef struct MvlptAugmentDesc {
  int32_t n_ops;            /* 0..4 colour operations, applied in the order of ops[] */
  int32_t ops[4];           /* distinct MVLPT_AUG_* ids */
  float   factor[3];        /* brightness, contrast, saturation factor (finite, >= 0), read only if the operation is listed */
  int32_t hue_shift;        /* 0..255, added to H modulo 256; read only if hue is listed */
  int32_t grayscale;        /* 1: replace the image by its L channel after the colour operations */
  int32_t n_holes;          /* 0..MVLPT_AUG_MAX_HOLES */
  int32_t hole[MVLPT_AUG_MAX_HOLES][4];   /* top, left, height >= 1, width >= 1, inside the output window (clipped by the caller) */
} MvlptAugmentDesc;
/* As mvlpt_preprocess, plus: aug: HOST array of B descriptors or NULL (no colour operation, grayscale or hole);
 * fill_outside 1: the window [out_top, out_top+out_h) x [out_left, out_left+out_w) may lie partly or wholly outside the resized image
 * (offsets within +-2^30), pixels outside are (0, 0, 0); 0: it must lie inside.  With aug == NULL and fill_outside == 0 the call IS
 * mvlpt_preprocess.  out_u8 is the 8-bit image just before ToTensor (after flip, colour operations, grayscale and holes).  Everything
 * the device indexes is checked on the host first: a bad descriptor returns MVLPT_ERR_ARG and nothing is launched.  B == 0 returns 0. */
int mvlpt_preprocess_aug(void* handle, const uint8_t* src, int64_t src_bytes, const MvlptImageDesc* descs, const MvlptAugmentDesc* aug,
                         int B, int out_h, int out_w, int fill_outside, const float* mean, const float* std, void* out, int out_dtype,
                         uint8_t* out_u8, mvlpt_stream_t stream);

/* ---- baseline JPEG decode on the device (row f3c of the scope table) -----------------------------------------
 * Compressed files -> the packed uint8 HWC RGB buffer mvlpt_preprocess(_aug) reads (MvlptImageDesc.offset), bit-identical to
 * Pillow's `Image.open(f).convert("RGB")` (libjpeg-turbo: Huffman decode, jidctint "islow" IDCT, fancy chroma upsampling, 16-bit
 * fixed-point YCbCr -> RGB; EXIF orientation is not applied, as Pillow does not on open).
 * The device decodes one SOF0 frame (baseline, Huffman, 8-bit samples and tables) with one interleaved scan of one component
 * (grayscale, replicated to R = G = B) or of three taken as YCbCr (JFIF APP0 present or component ids 1, 2, 3; no Adobe APP14), luma
 * sampled 1x1, 2x1 or 2x2 with 1x1 chroma, with or without restart intervals.  Every other file is found by the host parser before
 * anything is launched and left to the caller (MVLPT_JPEG_ROUTE_*): nothing is emulated. */
enum {
  MVLPT_JPEG_ROUTE_DEVICE = 0,
  MVLPT_JPEG_ROUTE_MALFORMED = 1,   /* no SOI, a marker where none may stand, a marker length past the file, no frame / scan header */
  MVLPT_JPEG_ROUTE_FRAME = 2,       /* not SOF0 / 8 bit: progressive, arithmetic, extended (SOF1), lossless, 12-bit */
  MVLPT_JPEG_ROUTE_SCANS = 3,       /* several scans, a scan that does not interleave all components, DNL */
  MVLPT_JPEG_ROUTE_COLOUR = 4,      /* CMYK / YCCK, Adobe APP14, RGB-tagged components */
  MVLPT_JPEG_ROUTE_SAMPLING = 5,    /* other sampling factors (4:4:0, 4:1:1, ...) */
  MVLPT_JPEG_ROUTE_TABLES = 6,      /* a table the scan names is missing, 16-bit, outside baseline's ids, or not a prefix code */
  MVLPT_JPEG_ROUTE_RESTART = 7,     /* RSTn out of sequence, or not ceil(MCUs / DRI) - 1 of them */
  MVLPT_JPEG_ROUTE_SIZE = 8         /* an empty image, one above 2^26 pixels, or a file of 2 GiB or more */
};
/* bits of a status word > 0 (corrupt entropy data; the segment it was met in stops, its remaining coefficients are 0) */
#define MVLPT_JPEG_ST_BAD_CODE 1     /* the next 16 bits match no Huffman code */
#define MVLPT_JPEG_ST_COEF_INDEX 2   /* a run carries the coefficient index past 63 */
#define MVLPT_JPEG_ST_ENDED_EARLY 4  /* the segment's bytes ran out before its MCUs did (zeros were fed) */
#define MVLPT_JPEG_ST_BAD_SIZE 8     /* a DC size above 15 */
typedef struct MvlptJpegInfo {
  int32_t height, width, components;   /* as the frame header gives them; 0 when it was not reached */
  int32_t h_samp, v_samp;              /* sampling factors of the first component */
  int32_t restart_interval;            /* DRI, in MCUs; 0: none */
  int32_t n_segments;                  /* restart segments of the scan (1 without DRI); 0 unless route == MVLPT_JPEG_ROUTE_DEVICE */
  int32_t route;                       /* MVLPT_JPEG_ROUTE_* */
} MvlptJpegInfo;
/* Host only, no handle, no device: reads the headers of the n bytes at `bytes`, never outside [0, n), and delimits the restart segments. */
int mvlpt_jpeg_probe(const uint8_t* bytes, int64_t n, MvlptJpegInfo* info);
/* Bytes of engine workspace a decode of these B files takes (coefficient blocks, component planes, descriptors and tables of the files
 * whose route is DEVICE).  The engine reserves it itself (grow-only); the figure is for planning. */
int mvlpt_jpeg_workspace_bytes(const MvlptJpegInfo* infos, int B, int64_t* bytes);
/* Decodes B files.  src_host / src_dev: the same compressed bytes in host and device memory, file b at [src_offsets[b], + src_sizes[b])
 * of both (host arrays).  The host parses, uploads table sets, segment and image descriptors and the initial status on `stream`, and
 * launches entropy decode, IDCT and upsample / colour for the files whose route is DEVICE; file b's pixels go to dst_dev +
 * dst_offsets[b] as uint8 [height, width, 3].  The others are skipped (the caller decodes them and writes their pixels there).
 * status_dev: int32 [B] on the device: 0 decoded, > 0 corrupt entropy data (MVLPT_JPEG_ST_*; the pixels are what the damaged data
 * gives, in bounds), -1 left to the host.  Enqueue-only: nothing is read back.  Everything the device indexes is checked on the host
 * first: a descriptor that would reach outside [0, dst_bytes), a negative offset or size, or B > 16384 returns MVLPT_ERR_ARG with
 * nothing launched.  B == 0 returns 0. */
int mvlpt_jpeg_decode(void* handle, const uint8_t* src_host, const uint8_t* src_dev, const int64_t* src_offsets, const int64_t* src_sizes,
                      int B, uint8_t* dst_dev, int64_t dst_bytes, const int64_t* dst_offsets, int32_t* status_dev, mvlpt_stream_t stream);
/* The three stages on their own (kernel-level tests; handle-free, enqueue-only).
 *   mvlpt_op_jpeg_entropy: one file whose route is DEVICE (MVLPT_ERR_UNSUPPORTED otherwise), n bytes at file_host and file_dev.  coefs:
 *     device int16 [coef_blocks][64], natural order, component after component, each raster over its whole-MCU block grid; zeroed and
 *     filled by the call; coef_blocks must be the file's block count.  ws / ws_bytes: device scratch for descriptor, tables and segment
 *     table, at least 4096 + 8 * n_segments bytes.  status_dev: one int32.
 *   mvlpt_op_jpeg_idct: coefs int16 [n_blocks][64] x quant uint8 [64] (natural order, device) -> plane uint8 [n_blocks / blocks_w * 8]
 *     [blocks_w * 8]; n_blocks % blocks_w == 0; plane 8-byte aligned.
 *   mvlpt_op_jpeg_colour: planes of `components` (1 or 3) components at planes + plane_off[c] with pitch plane_w[c] (host arrays; luma at
 *     least height x width, chroma at least ceil(height / vs) x ceil(width / hs)), luma factors hs x vs in {1x1, 2x1, 2x2} -> dst uint8
 *     [height, width, 3]. */
int mvlpt_op_jpeg_entropy(const uint8_t* file_host, int64_t n, const uint8_t* file_dev, void* ws, int64_t ws_bytes, int16_t* coefs,
                          int64_t coef_blocks, int32_t* status_dev, mvlpt_stream_t stream);
int mvlpt_op_jpeg_idct(const int16_t* coefs, const uint8_t* quant, int n_blocks, int blocks_w, uint8_t* plane, mvlpt_stream_t stream);
int mvlpt_op_jpeg_colour(const uint8_t* planes, const int64_t* plane_off, const int32_t* plane_w, int components, int hs, int vs, int height,
                         int width, uint8_t* dst, mvlpt_stream_t stream);

/* ---- per-kernel timing with HIP events on the launch stream (bench.py's roofline leg) --------------------- */
typedef struct MvlptKernelStat {
  char name[32];
  int64_t launches;
  double ms;    /* sum of event-timed launch durations */
  double flops; /* algorithmic FLOPs summed over launches (2*M*N*K for GEMM, 4*L*L*64 per head for attention) */
  double bytes; /* algorithmic HBM bytes summed over launches */
  double busy_ms; /* length of the UNION of the launch intervals: equals `ms` when launches never overlap; smaller
                     when the same kernel runs concurrently on two streams (image and text tower) */
  double flops_executed; /* FLOPs the launches actually issued: 2x `flops` for GEMMs with split-precision operands */
} MvlptKernelStat;
/* all_kernels == 0: only the dominant kernel (gemm_bt) is timed, through its own dispatch timestamps (no marker
 * packets on the stream); != 0: every kernel class is bracketed by marker events (adds ~1.5 us per event). */
int mvlpt_profile_begin(void* handle, int all_kernels);
/* paused != 0: launches are not timed until resumed (bench.py samples every 4th step to keep the overhead ~1 %) */
int mvlpt_profile_pause(void* handle, int paused);
/* synchronises the recorded events, fills up to `max_stats` entries, returns the number written (or <0): first one entry per kernel
 * class (busy_ms = union of the launch intervals), then the GEMM launches once more per problem, longest total time first, named
 * "g<M>x<N>x<K> e<epilogue> s<operand format> f<folded consumer>" (busy_ms = ms = sum of the launch durations) */
int mvlpt_profile_end(void* handle, MvlptKernelStat* stats, int max_stats);

#ifdef __cplusplus
}
#endif
#endif /* MVLPT_HIP_H */
