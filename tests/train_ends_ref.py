"""Plain-torch statements of the kernels at the two ends of a training step, and the case tables of tests/test_gpu_train_ends_ops.py:
the Baseline head (csrc/baseline.hip), BCE-with-logits and the multi-tensor SGD / Adam (csrc/optim.hip), the dropout passes
(csrc/dropout.hip) and the fixed-order BatchNorm sums (mt_det_bn_sums, csrc/det.hip).  Every function is the operation's definition
(torch modules, torch.optim, autograd) in the dtype of its arguments -- fp64 in the tests, fp32 for the yardstick -- on the CPU; nothing
here imports the library.  tests/test_train_ends_ref_host.py holds each one against an independent statement of the same operation and
asserts that the tables below contain every edge they were written for."""
import math

import torch
import torch.nn.functional as Fn

# ---- case tables ----------------------------------------------------------------------------------------------------------------

HEAD_CHUNK, HEAD_SLAB, HEAD_PREP_COLS, HEAD_PREP_GROUPS = 256, 32, 64, 16        # csrc/baseline.hip: kChunk, kSlab, prep's block
HEAD_CASES = [(1, 1, 4, 1),           # (n, hw, C, m): the minimum
              (3, 49, 260, 17),       # second chunk of 4 channels; row groups 9..15 empty (per = 2)
              (33, 64, 256, 5),       # c == C in a block of its own in prep and slab; exactly one NCHW lane pass; two slabs
              (2, 100, 64, 40),       # NCHW second lane pass; prep's c == C is lane 0 of block 2
              (65, 9, 508, 16),       # hw % 4 != 0; 252-channel tail; three slabs, the last of one crop
              (2, 3, 1280, 512)]      # the model's dims with hw < 4
HEAD_LAYOUTS = (0, 1)                 # NHWC, NCHW
HEAD_REGIMES = ("moderate", "offset")

BCE_N = (1, 63, 64, 255, 256, 257, 1000)
BCE_POS_WEIGHT = (1.0, 2.5, 0.4)
BCE_LABELS = ("hard", "soft")
BCE_REGIMES = ("moderate", "saturated", "tiny")
BCE_SATURATED = (30.0, 88.0, 89.0, 104.0, 230.0)      # either side of expf overflow (88.7) and of flush-to-zero (e^-104 < 2^-149)

OPT_CHUNK = 4096                      # csrc/optim.hip SGD_CHUNK
OPT_SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8193)
# (numel, offset of p, offset of g) -- offsets in floats from a 16-byte boundary; m and v of Adam sit at the offsets of g and p swapped
OPT_TABLES = {
    "sizes": [(4, 0, 0), (4096, 3, 1), (4096, 0, 0), (3, 2, 2), (5, 0, 0), (4095, 0, 0), (4097, 0, 0), (8193, 0, 0), (1, 0, 0), (5, 0, 3),
              (4095, 2, 1), (4097, 0, 2), (8193, 2, 0), (3, 1, 0)],
    "empties": [(0, 1, 1), (4097, 0, 0), (0, 2, 2), (0, 3, 1), (5, 0, 0), (4096, 3, 2), (0, 1, 0)],
}
SGD_WD = (0.0, 1e-2)
ADAM_STEPS = (1, 2, 1000)
ADAM_GRAD_SCALES = (1e-12, 1e-6, 1.0, 1e6)

MUL_PLANES_CASES = [(1, 8), (31, 8), (33, 24), (5, 20), (64, 136), (100, 72)]     # (rows, cols)
MUL_ADD_GRID, MUL_ADD_BLOCK = 8192, 256                                           # csrc/dropout.hip: the grid is capped at 8192 blocks
MUL_ADD_N = (4, 1028, 4 * 256 * 8192 + 4)
GEGLU_N_HALF = (8, 24, 72)
GEGLU_ROWS = (1, 33, 100)
GEGLU_REGIMES = ("moderate", "tails", "tiny")

BN_ROWS_PER_BLOCK = 2048              # csrc/det.hip kBnRowsPerBlock
BN_C = (1, 16, 17, 32, 33, 64, 65, 100)
BN_ROWS = (1, 15, 2047, 2048, 2049, 4097)
BN_CASES = [(rows, C) for C in BN_C for rows in (1, 4097)] + [(rows, C) for rows in (15, 2047, 2048, 2049) for C in (1, 17, 32, 100)]
BN_REGIMES = ("moderate", "offset")


def bn_width(C):
    """The instantiation mt_det_bn_sums selects (columns per block)."""
    return 16 if C <= 16 else 32 if C <= 32 else 64


def carve(entries):
    """Float offsets of the tensors of an OPT_TABLES entry inside two arenas that start on a 16-byte boundary: each tensor starts at
    the first position past its predecessor that leaves at least one float free and has the asked-for offset from a 16-byte boundary.
    Returns (p_starts, g_starts, p_total, g_total); totals include a trailing gap."""
    out = []
    for which in (1, 2):
        cur, starts = 0, []
        for e in entries:
            pos = cur + 1
            while pos % 4 != e[which]:
                pos += 1
            if not starts:
                pos = e[which]
            starts.append(pos)
            cur = pos + e[0]
        out.append((starts, cur + 2))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def gaps(entries, starts):
    """The number of free floats between each tensor and its successor."""
    return [starts[k + 1] - (starts[k] + entries[k][0]) for k in range(len(entries) - 1)]


# ---- the Baseline head ----------------------------------------------------------------------------------------------------------

def _head_logits(x, layout, w1, b1, w2, b2):
    """x: [n, hw, C] (layout 0) or [n, C, hw] (layout 1).  AdaptiveAvgPool2d(1) -> Linear(C, m) -> Linear(m, 1)."""
    img = (x.permute(0, 2, 1) if layout == 0 else x).unsqueeze(-1)                 # [n, C, hw, 1]
    pooled = Fn.adaptive_avg_pool2d(img, 1).flatten(1)
    return _mlp(pooled, w1, b1, w2, b2), pooled


def _mlp(pooled, w1, b1, w2, b2):
    return Fn.linear(Fn.linear(pooled, w1, b1), w2.reshape(1, -1), b2.reshape(1)).reshape(-1)


def baseline_head(x, layout, w1, b1, w2, b2):
    """-> logits [n], pooled [n, C], v [C], c0 (0-dim).  v and c0 are read off the definition: the two Linears at pooled = 0 give c0,
    and their Jacobian with respect to pooled (autograd) gives v."""
    logits, pooled = _head_logits(x, layout, w1, b1, w2, b2)
    zero = torch.zeros(1, w1.shape[1], dtype=x.dtype, requires_grad=True)
    at0 = _mlp(zero, w1, b1, w2, b2)
    v = torch.autograd.grad(at0.sum(), zero)[0].reshape(-1)
    return logits.detach(), pooled.detach(), v, at0.detach().reshape(())


def baseline_head_bwd(x, layout, w1, b1, w2, b2, dlogits):
    """Autograd of the definition: {dW1 [m, C], db1 [m], dW2 [m], db2 [1], dx (x's shape)} for the loss sum_i dlogits_i logit_i."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    logits, _ = _head_logits(leaves[0], layout, *leaves[1:])
    dx, dw1, db1, dw2, db2 = torch.autograd.grad((logits * dlogits).sum(), leaves)
    return {"dW1": dw1, "db1": db1, "dW2": dw2.reshape(-1), "db2": db2.reshape(1), "dx": dx}


def head_inputs(n, hw, C, m, layout, regime, seed):
    """fp32 (x, w1, b1, w2, b2, dlogits).  `offset`: features with mean 1e3 and standard deviation 1 (post-activation features are not
    centred).  dlogits holds one exact zero when there is more than one crop (with a single crop it would zero every gradient)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, hw, C) if layout == 0 else (n, C, hw), generator=g)
    if regime == "offset":
        x = x + 1000.0
    w1, b1 = torch.randn(m, C, generator=g) * C ** -0.5, torch.randn(m, generator=g) * 0.1
    w2, b2 = torch.randn(m, generator=g) * m ** -0.5, torch.randn(1, generator=g)
    dl = torch.randn(n, generator=g)
    if n > 1:
        dl[n // 2] = 0.0
    return x, w1, b1, w2, b2, dl


# ---- BCE with logits ------------------------------------------------------------------------------------------------------------

def bce_with_logits(x, y, pos_weight):
    """-> (loss (0-dim), dloss/dx [n]) of BCEWithLogitsLoss(pos_weight) with mean reduction."""
    xl = x.detach().clone().requires_grad_(True)
    loss = Fn.binary_cross_entropy_with_logits(xl, y, pos_weight=torch.tensor([pos_weight], dtype=x.dtype))
    return loss.detach(), torch.autograd.grad(loss, xl)[0]


def bce_inputs(n, regime, labels, seed):
    g = torch.Generator().manual_seed(seed)
    if regime == "moderate":
        x = torch.randn(n, generator=g) * 4
    elif regime == "tiny":
        x = torch.randn(n, generator=g) * 1e-6
    else:
        mags = torch.tensor(BCE_SATURATED)
        x = mags[torch.arange(n) % len(mags)] * (1.0 - 2.0 * ((torch.arange(n) // len(mags)) % 2))
        x = x[torch.randperm(n, generator=g)]
    y = (torch.rand(n, generator=g) > 0.5).float()
    if labels == "soft":
        y = torch.where(torch.rand(n, generator=g) > 0.5, torch.full((n,), 0.3), y)
    if regime == "saturated":        # element 0 is saturated on the wrong side of its label: the largest gradient is O(1) at every n, n = 1 too
        y[0] = 1.0 if x[0] < 0 else 0.0
    return x, y


# ---- optimizers -----------------------------------------------------------------------------------------------------------------

def sgd_step(p, g, lr, wd):
    """One torch.optim.SGD(lr, weight_decay = wd) step (no momentum) on a copy of p."""
    q = torch.nn.Parameter(p.detach().clone())
    q.grad = g.detach().clone()
    torch.optim.SGD([q], lr=lr, weight_decay=wd).step()
    return q.detach()


def adam_step(p, g, m, v, lr, wd, t, decoupled):
    """Step number t (1-based) of torch.optim.Adam (decoupled = False) / AdamW (True) with the default betas and eps, from the
    moments m, v after step t - 1.  -> (p, m, v)."""
    q = torch.nn.Parameter(p.detach().clone())
    q.grad = g.detach().clone()
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([q], lr=lr, weight_decay=wd, foreach=False)
    st = opt.state[q]
    st["step"] = torch.tensor(float(t - 1))
    st["exp_avg"], st["exp_avg_sq"] = m.detach().clone(), v.detach().clone()
    opt.step()
    assert float(st["step"]) == t
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


def adam_bias_corrections(lr, t, betas=(0.9, 0.999)):
    """(step_size, bias_correction2_sqrt) as mintime_amd/optim.py computes them on the host (Python doubles)."""
    return lr / (1.0 - betas[0] ** t), (1.0 - betas[1] ** t) ** 0.5


# ---- dropout passes -------------------------------------------------------------------------------------------------------------

def mul(x, m):
    return x * m


def mul_add(y, m, r):
    return r + y * m


def interleave(a, g):
    """u = (a_0, g_0, a_1, g_1, ...) per row, as the forward GEGLU epilogue stores the pre-activations."""
    return torch.stack([a, g], dim=-1).reshape(a.shape[0], 2 * a.shape[1])


def deinterleave(u):
    pair = u.reshape(u.shape[0], -1, 2)
    return pair[..., 0], pair[..., 1]


def geglu_bwd(dh, m, u_interleaved):
    """-> du [rows, 2 n_half] = [da | dg] of h = a * gelu(g) (exact erf) followed by the dropout multiplier m (None: no dropout),
    for the upstream gradient dh."""
    a, g = (t.detach().clone().requires_grad_(True) for t in deinterleave(u_interleaved))
    h = a * Fn.gelu(g)
    if m is not None:
        h = h * m
    da, dg = torch.autograd.grad((h * dh).sum(), (a, g))
    return torch.cat([da, dg], dim=1)


def geglu_inputs(rows, n_half, regime, seed):
    g_ = torch.Generator().manual_seed(seed)
    a = torch.randn(rows, n_half, generator=g_)
    if regime == "moderate":
        g = torch.randn(rows, n_half, generator=g_) * 1.5
    elif regime == "tails":
        g = (4.0 + 8.0 * torch.rand(rows, n_half, generator=g_)) * (1.0 - 2.0 * (torch.rand(rows, n_half, generator=g_) > 0.5).float())
    else:
        g = torch.randn(rows, n_half, generator=g_) * 1e-6
    dh = torch.randn(rows, n_half, generator=g_)
    m = (torch.rand(rows, n_half, generator=g_) > 0.3).float() / 0.7
    return dh, m, interleave(a, g).contiguous()


# ---- BatchNorm sums -------------------------------------------------------------------------------------------------------------

def bn_sums(x, z, mean_istd, mode, exact=False):
    """-> [2, C]: mode 0 = (sum x, sum x^2) over the rows; mode 1 = (sum x, sum x (z - mean) istd), mean_istd = [2, C].
    exact: the column sums are math.fsum's (correctly rounded whatever the order -- the kernel accumulates in fp64 too, so a torch
    sum's own rounding, which depends on the host's vector width, would be as large as what is being measured)."""
    t2 = x * x if mode == 0 else x * ((z - mean_istd[0]) * mean_istd[1])
    if not exact:
        return torch.stack([x.sum(0), t2.sum(0)])
    return torch.tensor([[math.fsum(col) for col in t.t().tolist()] for t in (x, t2)], dtype=x.dtype)


def bn_inputs(rows, C, regime, seed):
    """fp32 (x [rows, C], z [rows, C], mean_istd [2, C], start [2, C] fp64 -- the non-zero values the entry point accumulates onto)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 3 + 1 if regime == "moderate" else torch.randn(rows, C, generator=g) + 1000.0
    z = torch.randn(rows, C, generator=g) * 2 + 0.5
    mi = torch.stack([torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) + 0.5])
    start = torch.randn(2, C, generator=g, dtype=torch.float64)
    return x, z, mi, start
