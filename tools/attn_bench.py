"""Time attention fwd/bwd kernels (through the C ABI) on the step's shapes. GPU box only.

  python tools/attn_bench.py [--head-width W] [--reps 7]

--head-width W (80, 96, 112, 128): instead, time the wide-head forward (attention_wide.hip) at the ViT-H/14 shape (N 256, L 257,
d = 1280) against torch's scaled_dot_product_attention on the same tensors and against the 64-wide streaming forward at the same d
(H = d / 64), alternating the three rep by rep; prints the median, minimum and maximum of each and the ratios."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mvlpt_amd import engine as E

def timeit(fn, iters=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters

if "--head-width" in sys.argv:
    import statistics
    W = int(sys.argv[sys.argv.index("--head-width") + 1])
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    N, L, d = 256, 257, 1280
    H, H64 = d // W, d // 64
    qkv = torch.randn(N * L, 3 * d, device="cuda").half()
    out = torch.empty(N * L, d, device="cuda", dtype=torch.float16)
    q, k, v = (t.reshape(N, L, H, W).transpose(1, 2) for t in qkv.view(N * L, 3, d).unbind(1))      # views: no copy inside the timing
    fns = {"wide": lambda: E.op_attention_wide_fwd(qkv, N, L, H, W, want_lse=False, out=out),
           "sdpa": lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v),
           "stream64": lambda: E.op_attention_fwd(qkv, N, L, H64, False, want_lse=False)}
    ms = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            ms[n].append(timeit(fn))
    med = {n: statistics.median(t) for n, t in ms.items()}
    fl = {"wide": 4.0 * L * L * W * N * H, "sdpa": 4.0 * L * L * W * N * H, "stream64": 4.0 * L * L * 64 * N * H64}
    for n in fns:
        print(f"{n:9s} N={N} L={L} d={d} w={64 if n == 'stream64' else W}: median {med[n]*1e3:7.1f} us (min {min(ms[n])*1e3:7.1f}, max {max(ms[n])*1e3:7.1f}; "
              f"{reps} reps) {fl[n]/med[n]/1e9:6.1f} TF")
    print(f"wide / sdpa = {med['wide'] / med['sdpa']:.3f}   wide / stream64 = {med['wide'] / med['stream64']:.3f}")
    sys.exit(0)

for (N, L, H, causal) in [(256, 197, 12, False), (256, 205, 12, False), (256, 50, 12, False), (100, 77, 8, True), (1000, 77, 8, True),
                          (128, 261, 16, False), (128, 581, 16, False)]:
    d = H * 64
    qkv = torch.randn(N * L, 3 * d, device="cuda").half()
    out, lse = E.op_attention_fwd(qkv, N, L, H, causal)
    dout = torch.randn(N * L, d, device="cuda").half()
    tf = timeit(lambda: E.op_attention_fwd(qkv, N, L, H, causal))
    tb = timeit(lambda: E.op_attention_bwd(qkv, out, dout, lse, N, L, H, causal))
    fl = 4.0 * L * L * 64 * N * H * (0.5 if causal else 1.0)
    print(f"N={N} L={L} H={H} causal={causal}: fwd {tf*1e3:7.1f} us ({fl/tf/1e9:6.1f} TF)  bwd {tb*1e3:7.1f} us ({2.5*fl/tb/1e9:6.1f} TF)")

print("split-precision attention (hi|lo pair operands, three-term products; kernels only, outputs preallocated):")
from mvlpt_amd import _lib
for (N, L, H, causal) in [(256, 205, 12, False), (100, 77, 8, True), (2191, 77, 8, True), (128, 581, 16, False)]:
    d = H * 64
    qkv = E.split_pair(torch.randn(N * L, 3 * d, device="cuda"), torch.float16)
    out, lse = E.op_attention32_fwd_pair(qkv, N, L, H, causal)
    dout = E.split_pair(torch.randn(N * L, d, device="cuda"), torch.float16)
    dqkv = torch.empty(N * L, 6 * d, device="cuda", dtype=torch.float16)
    delta = torch.empty(N * H * L, device="cuda", dtype=torch.float32)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()
    tf = timeit(lambda: _lib.lib.mvlpt_op_attention32_fwd(1, P(qkv), P(out), P(lse), N, L, H, int(causal), 0, st))
    tb = timeit(lambda: _lib.lib.mvlpt_op_attention32_bwd(1, P(qkv), P(out), P(dout), P(lse), P(delta), P(dqkv), N, L, H, int(causal), st))
    fl = 4.0 * L * L * 64 * N * H * (0.5 if causal else 1.0)
    print(f"N={N} L={L} H={H} causal={causal}: fwd {tf*1e3:7.1f} us ({fl/tf/1e9:6.1f} TF)  bwd {tb*1e3:7.1f} us ({2.5*fl/tb/1e9:6.1f} TF)")
