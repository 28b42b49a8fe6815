"""Float64 references and derived error bounds of the zero-shot glue kernels (mvlpt_amd/csrc/glue.hip: embed_tokens_kernel,
ensemble_features_kernel).  Plain torch on whatever device the tensors live on; nothing here launches a kernel of the library.
tests/test_zsclip_host.py checks the module without a GPU, tests/test_hip_zsclip_ops.py uses it.

embed_tokens.  x[s, t] = emb[ids[s, t]] + pos[t]: ONE fp32 addition per element, and IEEE addition is correctly rounded, so the float64
sum rounded to fp32 IS the result: the test asserts bit equality, there is no bound.

ensemble_features.  out[c] = normalize((1 / T) sum_t feats[t, c] / |feats[t, c]|), reference in float64.  Per-element bound, first order in
u = 2^-24 (fp32, round to nearest), valid for any order of the sums of squares (their terms are non-negative):
  |x|^2 over e terms (products rounded, then e - 1 additions in any order)      relative error <= (e + 1) u, so <= (e + 1) u / 2 on |x|
  sqrt and division: correctly rounded (<= u) under hipcc's default; U_DIV_SQRT = 2 u each is allowed here so that the bound does not
  lean on that compiler default
  unit vector v = x / |x|:                       eps_v = ((e + 1) / 2) u + 2 U_DIV_SQRT                 (relative, per element)
  acc = sum_t v_t, sequential over t = 0..T-1:   E_acc = (eps_v + (T - 1) u) A,  A = sum_t |v_t|         (per element)
  m = acc / T:                                   E_m = E_acc / T + U_DIV_SQRT |m|
  out = m / |m|:                                 |d out_k| <= E_m_k / |m| + |out_k| (||E_m||_2 / |m| + ((e + 1) / 2) u + 2 U_DIV_SQRT)
(the norm is 1-Lipschitz, so an error vector E_m moves |m| by at most its 2-norm).  The neglected second-order terms are below
e u ~ 5e-5 of the bound at e = 768; SECOND_ORDER = 1.001 covers them.  Nothing in the bound is measured: there is no transcendental
function in the kernel.  For T = 1 the kernel skips the second normalisation (the mean of one unit vector is that vector), which only
removes terms."""
import torch

U32 = 2.0 ** -24
U_DIV_SQRT = 2.0 * U32
SECOND_ORDER = 1.001


def embed_ref64(emb, pos, ids, L):
    """float64 [S, L, d] from fp32 emb [V, d], pos [>= L, d] and integer ids [S, ld] (columns 0 .. L-1 are read)."""
    idx = ids[:, :L].long()
    return emb.double()[idx] + pos.double()[:L]


def ensemble_ref64(feats):
    """float64 [C, e] from feats [T, C, e] (trainers/zsclip.py:88-96)."""
    f = feats.double()
    v = f / f.norm(dim=-1, keepdim=True)
    m = v.sum(0) / f.shape[0]
    return m / m.norm(dim=-1, keepdim=True)


def ensemble_bound(feats):
    """Per-element bound [C, e] (float64) on |fp32 result - ensemble_ref64(feats)|; see the module docstring."""
    f = feats.double()
    T, _, e = f.shape
    half_norm = 0.5 * (e + 1) * U32
    eps_v = half_norm + 2 * U_DIV_SQRT
    v = f / f.norm(dim=-1, keepdim=True)
    A = v.abs().sum(0)
    m = v.sum(0) / T
    E_m = (eps_v + (T - 1) * U32) * A / T + U_DIV_SQRT * m.abs()
    n2 = m.norm(dim=-1, keepdim=True)
    out = m / n2
    bound = E_m / n2 + out.abs() * (E_m.norm(dim=-1, keepdim=True) / n2 + half_norm + 2 * U_DIV_SQRT)
    return SECOND_ORDER * bound


def ensemble_inputs(T, C, e, seed=0):
    """Seeded fp32 features [T, C, e] with rows of very different length (the normalisation must not care) and a common direction per
    class plus template noise, as real template features have."""
    g = torch.Generator().manual_seed(7919 * T + 131 * C + e + seed)
    base = torch.randn(1, C, e, generator=g)
    noise = torch.randn(T, C, e, generator=g)
    scale = torch.exp(torch.randn(T, C, 1, generator=g) * 2.0)
    return ((base + 0.7 * noise) * scale).float()
