"""tests/train_ends_ref.py against independent fp64 statements of the same operations (CPU): the Baseline head's rank-1 algebra as
csrc/baseline.hip's header comment writes it, the closed-form BCE gradient of csrc/optim.hip's comment, hand-written SGD / Adam / AdamW
steps, the GEGLU gradient written out with erf, loops for the BatchNorm sums.  Everything is fp64, so the bound is rounding of fp64
sums.  The second half asserts the coverage facts of the case tables tests/test_gpu_train_ends_ops.py runs: every edge the tables were
written for is named here, so an edit of a table cannot silently drop one."""
import math

import pytest
import torch

from . import train_ends_ref as R
from .util import rel_err

TOL = 1e-12      # fp64: sums of up to ~1e5 terms in two different orders differ by ~1e-13 relative at the most


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


# ---- the references ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", R.HEAD_LAYOUTS)
@pytest.mark.parametrize("n,hw,C,m", R.HEAD_CASES)
def test_head_reference_is_the_rank_one_form(n, hw, C, m, layout):
    """v = W1^T w2, c0 = w2 . b1 + b2, logit_i = mean_p(x_i[p, :]) . v + c0;  s = sum g, u = sum_i g_i pooled_i, db2 = s, db1 = w2 s,
    dW1 = w2 (x) u, dW2[j] = W1[j, :] . u + b1[j] s, dx_i[p, c] = g_i v[c] / hw."""
    x, w1, b1, w2, b2, dl = (t.double() for t in R.head_inputs(n, hw, C, m, layout, "moderate", 5))
    logits, pooled, v, c0 = R.baseline_head(x, layout, w1, b1, w2, b2)
    pooled_rank1 = x.sum(1) / hw if layout == 0 else x.sum(2) / hw
    v_rank1, c0_rank1 = w1.t() @ w2, w2 @ b1 + b2[0]
    assert rel_err(pooled, pooled_rank1) <= TOL and rel_err(v, v_rank1) <= TOL and rel_err(c0, c0_rank1) <= TOL
    assert rel_err(logits, pooled_rank1 @ v_rank1 + c0_rank1) <= TOL
    gr = R.baseline_head_bwd(x, layout, w1, b1, w2, b2, dl)
    s, u = dl.sum(), dl @ pooled_rank1
    assert rel_err(gr["db2"], s.reshape(1)) <= TOL and rel_err(gr["db1"], w2 * s) <= TOL
    assert rel_err(gr["dW1"], torch.outer(w2, u)) <= TOL and rel_err(gr["dW2"], w1 @ u + b1 * s) <= TOL
    dx = dl[:, None, None] * (v_rank1[None, None, :] if layout == 0 else v_rank1[None, :, None]) / hw
    assert rel_err(gr["dx"], dx.expand_as(x)) <= TOL
    if n > 1:
        assert float(dl[n // 2]) == 0.0 and int((dl == 0).sum()) == 1


@pytest.mark.parametrize("labels", R.BCE_LABELS)
@pytest.mark.parametrize("regime", R.BCE_REGIMES)
@pytest.mark.parametrize("pw", R.BCE_POS_WEIGHT)
def test_bce_reference_is_the_closed_form(pw, regime, labels):
    """loss = mean_i (1 - y) x + (1 + (pw - 1) y) softplus(-x);  dloss/dx_i = ((1 - y) - (1 + (pw - 1) y) sigmoid(-x)) / n."""
    n = 257
    x, y = (t.double() for t in R.bce_inputs(n, regime, labels, 3))
    loss, dx = R.bce_with_logits(x, y, pw)
    lw = 1.0 + (pw - 1.0) * y
    softplus_neg = torch.log1p(torch.exp(-x.abs())) + torch.clamp(-x, min=0.0)
    assert rel_err(loss, ((1.0 - y) * x + lw * softplus_neg).mean()) <= TOL
    assert rel_err(dx, ((1.0 - y) - lw / (1.0 + torch.exp(x))) / n) <= TOL
    assert torch.isfinite(loss) and torch.isfinite(dx).all()
    if regime == "saturated":
        assert {abs(float(v)) for v in x} == set(R.BCE_SATURATED) and bool((x > 0).any()) and bool((x < 0).any())
    if labels == "soft":
        assert bool((y == float(torch.tensor(0.3))).any()) and bool((y == 0).any()) and bool((y == 1).any())


@pytest.mark.parametrize("wd", R.SGD_WD)
def test_sgd_reference_is_the_written_out_step(wd):
    g = _g(1)
    p, gr = _rn(g, 301), _rn(g, 301)
    assert rel_err(R.sgd_step(p, gr, 0.1, wd), p - 0.1 * (gr + wd * p)) <= TOL
    assert torch.equal(R.sgd_step(p, gr, 0.0, wd), p)


@pytest.mark.parametrize("t", R.ADAM_STEPS)
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("decoupled", [False, True])
def test_adam_reference_is_the_written_out_step(decoupled, wd, t):
    """One Adam / AdamW step by hand (Kingma & Ba, algorithm 1; Loshchilov & Hutter for the decoupled decay), betas (0.9, 0.999),
    eps 1e-8, and the bias corrections the way mintime_amd/optim.py passes them."""
    g = _g(10 + t)
    p, gr, m0 = _rn(g, 200), _rn(g, 200) * 10.0 ** torch.randint(-12, 7, (200,), generator=g).double(), _rn(g, 200) * 0.1
    v0 = _rn(g, 200).abs() * 0.01
    lr, b1, b2, eps = 0.05, 0.9, 0.999, 1e-8
    q = p * (1.0 - lr * wd) if decoupled else p
    ge = gr if decoupled else gr + wd * p
    m = b1 * m0 + (1 - b1) * ge
    v = b2 * v0 + (1 - b2) * ge * ge
    step_size, bc2_sqrt = R.adam_bias_corrections(lr, t)
    assert step_size == lr / (1 - b1 ** t) and bc2_sqrt == math.sqrt(1 - b2 ** t)
    want = q - step_size * m / (v.sqrt() / bc2_sqrt + eps)
    got_p, got_m, got_v = R.adam_step(p, gr, m0, v0, lr, wd, t, decoupled)
    assert rel_err(got_m, m) <= TOL and rel_err(got_v, v) <= TOL and rel_err(got_p, want) <= TOL
    # per element too: the large gradients must not hide the small ones
    assert float(((got_v - v).abs() / v).max()) <= TOL and float(((got_p - want).abs() / want.abs()).max()) <= TOL


@pytest.mark.parametrize("with_m", [True, False])
@pytest.mark.parametrize("regime", R.GEGLU_REGIMES)
def test_geglu_reference_and_the_interleaved_layout(regime, with_m):
    """u = (a_0, g_0, a_1, g_1, ...) round-trips; da = dh m gelu(g), dg = dh m a (Phi(g) + g phi(g)) with erf written out."""
    rows, nh = 33, 24
    dh, m, u = (t.double() for t in R.geglu_inputs(rows, nh, regime, 2))
    a, g = R.deinterleave(u)
    assert torch.equal(R.interleave(a, g), u) and torch.equal(u[:, 0::2], a) and torch.equal(u[:, 1::2], g)
    assert torch.equal(u[:, 6], a[:, 3]) and torch.equal(u[:, 7], g[:, 3])
    mm = m if with_m else torch.ones_like(m)
    Phi = 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0)))
    phi = torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
    du = R.geglu_bwd(dh, m if with_m else None, u)
    assert du.shape == (rows, 2 * nh)
    assert rel_err(du[:, :nh], dh * mm * g * Phi) <= TOL and rel_err(du[:, nh:], dh * mm * a * (Phi + g * phi)) <= TOL
    if regime == "tails":
        assert float(g.abs().min()) >= 4.0 and float(g.abs().max()) <= 12.0 and bool((g < 0).any()) and bool((g > 0).any())
    assert set(m.unique().tolist()) == {0.0, float(torch.tensor(1.0 / 0.7, dtype=torch.float32))}


def test_mul_references():
    g = _g(4)
    x, m, r = _rn(g, 7, 5), _rn(g, 7, 5), _rn(g, 7, 5)
    for i in range(7):
        for j in range(5):
            assert float(R.mul(x, m)[i, j]) == float(x[i, j]) * float(m[i, j])
            assert abs(float(R.mul_add(x, m, r)[i, j]) - (float(r[i, j]) + float(x[i, j]) * float(m[i, j]))) <= 1e-15


@pytest.mark.parametrize("mode", [0, 1])
def test_bn_sums_reference_against_loops(mode):
    rows, C = 15, 5
    x, z, mi, _ = (t.double() for t in R.bn_inputs(rows, C, "moderate", 1))
    got = R.bn_sums(x, z, mi, mode)
    exact = R.bn_sums(x, z, mi, mode, exact=True)
    assert exact.shape == got.shape == (2, C) and exact.dtype == torch.float64 and rel_err(got, exact) <= TOL
    for c in range(C):
        s1 = sum(float(x[r, c]) for r in range(rows))
        if mode == 0:
            s2 = sum(float(x[r, c]) ** 2 for r in range(rows))
        else:
            s2 = sum(float(x[r, c]) * (float(z[r, c]) - float(mi[0, c])) * float(mi[1, c]) for r in range(rows))
        assert abs(float(got[0, c]) - s1) <= TOL * abs(s1) + 1e-14 and abs(float(got[1, c]) - s2) <= TOL * abs(s2) + 1e-13


# ---- the case tables ----------------------------------------------------------------------------------------------------------------

def test_head_cases_cover_their_edges():
    cases = R.HEAD_CASES
    assert (1, 1, 4, 1) in cases                                                                    # the minimum
    assert any(C > R.HEAD_CHUNK and C % R.HEAD_CHUNK for _, _, C, _ in cases)                       # a partial second 256-channel chunk
    assert any(C > R.HEAD_CHUNK and C % R.HEAD_CHUNK == 4 for _, _, C, _ in cases)                  # ... of one float4
    assert any(C % R.HEAD_PREP_COLS == 0 for _, _, C, _ in cases)                                   # prep: c == C opens a block
    assert any(C % R.HEAD_PREP_COLS == 0 and C // R.HEAD_PREP_COLS == 1 for _, _, C, _ in cases)    # ... lane 0 of block 2
    assert any(C % 256 == 0 for _, _, C, _ in cases)                                                # slab / slab_sum: c == C opens a block
    assert any(C % 256 == 0 and n > R.HEAD_SLAB for n, _, C, _ in cases)                            # ... with slab_sum launched
    assert any(m < R.HEAD_PREP_GROUPS for *_, m in cases)
    assert any(m > R.HEAD_PREP_GROUPS and m % R.HEAD_PREP_GROUPS for *_, m in cases)
    assert any(m > R.HEAD_PREP_GROUPS and -(-m // R.HEAD_PREP_GROUPS) * (R.HEAD_PREP_GROUPS - 1) >= m for *_, m in cases)   # empty groups
    assert any(m == R.HEAD_PREP_GROUPS for *_, m in cases) and any(m % 4 for *_, m in cases)       # params: a 4-row block with a tail
    assert any(hw < 4 for _, hw, _, _ in cases) and any(hw > 64 for _, hw, _, _ in cases) and any(hw == 64 for _, hw, _, _ in cases)
    assert any(hw >= 4 and hw % 4 for _, hw, _, _ in cases)                                         # dfeat<1>: a float4 across two channels
    assert {-(-n // R.HEAD_SLAB) for n, *_ in cases} >= {1, 2, 3}                                   # direct u; slab_sum over 2 and 3
    assert any(n % R.HEAD_SLAB == 1 and n > 2 * R.HEAD_SLAB for n, *_ in cases)                     # a last slab of one crop
    assert any(n == R.HEAD_SLAB + 1 for n, *_ in cases)
    assert (2, 3, 1280, 512) in cases                                                               # the model's own dims
    assert all(C % 4 == 0 for _, _, C, _ in cases)
    assert set(R.HEAD_LAYOUTS) == {0, 1} and set(R.HEAD_REGIMES) == {"moderate", "offset"}


def test_bce_cases_cover_their_edges():
    assert set(R.BCE_N) >= {1, 63, 64, 255, 256, 257, 1000}          # one lane; the wave and block edges; four strides of the block
    assert any(n > 3 * 256 for n in R.BCE_N)
    assert 1.0 in R.BCE_POS_WEIGHT and any(w > 1 for w in R.BCE_POS_WEIGHT) and any(w < 1 for w in R.BCE_POS_WEIGHT)
    overflow, flush = math.log(torch.finfo(torch.float32).max), 149 * math.log(2.0)     # expf(x) = inf above; expf(-x) = 0 above
    s = R.BCE_SATURATED
    assert any(v < overflow for v in s) and any(overflow < v < flush for v in s) and any(v > flush for v in s) and max(s) >= 230
    assert max(v for v in s if v < overflow) == 88.0 and min(v for v in s if v > overflow) == 89.0
    assert set(R.BCE_REGIMES) == {"moderate", "saturated", "tiny"} and set(R.BCE_LABELS) == {"hard", "soft"}


def test_optimizer_tables_cover_their_edges():
    main = R.OPT_TABLES["sizes"]
    assert {e[0] for e in main} == set(R.OPT_SIZES) == {1, 3, 4, 5, 4095, 4096, 4097, 8193}
    assert {R.OPT_CHUNK - 1, R.OPT_CHUNK, R.OPT_CHUNK + 1, 2 * R.OPT_CHUNK + 1} <= set(R.OPT_SIZES)
    assert {(e[1] == 0, e[2] == 0) for e in main} == {(True, True), (True, False), (False, True), (False, False)}
    assert all(0 <= e[1] <= 3 and 0 <= e[2] <= 3 for t in R.OPT_TABLES.values() for e in t)
    both = {e[0] for e in main if e[1] == 0 and e[2] == 0}                     # the float4 path
    assert both >= {4, 5, 4095, 4096, 4097, 8193}                               # whole vectors only, and a 1 / 3 element tail, per chunk edge
    for n in (4095, 4096, 4097):                                                # ... and each chunk edge off the float4 path too
        assert any(e[0] == n and (e[1] or e[2]) for e in main)
    for name, t in R.OPT_TABLES.items():
        ps, gs, ptot, gtot = R.carve(t)
        assert all(s % 4 == e[1] for s, e in zip(ps, t)) and all(s % 4 == e[2] for s, e in zip(gs, t))
        assert all(1 <= d <= 3 for d in R.gaps(t, ps) + R.gaps(t, gs)), name    # one to three guard floats between neighbours
        assert ptot >= ps[-1] + t[-1][0] + 1 and gtot >= gs[-1] + t[-1][0] + 1
    e = [x[0] for x in R.OPT_TABLES["empties"]]
    assert e[0] == 0 and e[-1] == 0 and e[1] > 0 and e[-2] > 0                  # empty first and last, real neighbours
    assert any(e[k] == 0 and e[k + 1] == 0 and e[k - 1] > 0 and e[k + 2] > 0 for k in range(1, len(e) - 2))      # two in the middle
    assert any(n > R.OPT_CHUNK for n in e)                                      # a neighbour of more than one block
    assert set(R.SGD_WD) == {0.0, 1e-2} and set(R.ADAM_STEPS) == {1, 2, 1000}
    assert min(R.ADAM_GRAD_SCALES) == 1e-12 and max(R.ADAM_GRAD_SCALES) == 1e6


def test_dropout_cases_cover_their_edges():
    mp = R.MUL_PLANES_CASES
    assert set(mp) == {(1, 8), (31, 8), (33, 24), (5, 20), (64, 136), (100, 72)}
    assert any(c % 8 for _, c in mp) and any(c % 16 == 8 for _, c in mp)        # off the lane width; half a 16-column block
    assert any(c > 64 for _, c in mp)                                           # more than one block of four 16-column wavefronts
    assert any(r < 32 for r, _ in mp) and any(r % 32 == 0 for r, _ in mp) and any(r > 32 and r % 32 for r, _ in mp)
    assert min(R.MUL_ADD_N) == 4 and all(n % 4 == 0 for n in R.MUL_ADD_N)
    assert max(R.MUL_ADD_N) // 4 == R.MUL_ADD_GRID * R.MUL_ADD_BLOCK + 1        # one float4 into the second trip of the grid-stride loop
    assert any(n // 4 % R.MUL_ADD_BLOCK and n // 4 > R.MUL_ADD_BLOCK for n in R.MUL_ADD_N)
    assert set(R.GEGLU_N_HALF) == {8, 24, 72} and all(h % 8 == 0 for h in R.GEGLU_N_HALF)
    assert any(h % 16 for h in R.GEGLU_N_HALF)                                  # the halves meet inside a 16-column block
    assert set(R.GEGLU_ROWS) == {1, 33, 100} and set(R.GEGLU_REGIMES) == {"moderate", "tails", "tiny"}


def test_bn_sums_cases_cover_their_edges():
    assert set(R.BN_C) == {1, 16, 17, 32, 33, 64, 65, 100} and set(R.BN_ROWS) == {1, 15, 2047, 2048, 2049, 4097}
    assert {C for _, C in R.BN_CASES} == set(R.BN_C) and {r for r, _ in R.BN_CASES} == set(R.BN_ROWS)
    assert {R.bn_width(C) for _, C in R.BN_CASES} == {16, 32, 64}
    for W in (16, 32, 64):
        mine = [(r, C) for r, C in R.BN_CASES if R.bn_width(C) == W]
        assert any(C % W for _, C in mine) and any(C == W for _, C in mine)                      # a partial column block; a full one
        assert any(r == 1 for r, _ in mine) and any(r > 2 * R.BN_ROWS_PER_BLOCK for r, _ in mine)  # one row; three chunks
    assert any(C > 64 for _, C in R.BN_CASES)                                                    # two column blocks of the widest
    for r in (R.BN_ROWS_PER_BLOCK - 1, R.BN_ROWS_PER_BLOCK, R.BN_ROWS_PER_BLOCK + 1):
        assert any(rows == r and R.bn_width(C) == 32 for rows, C in R.BN_CASES)                  # the chunk edge on the <32> kernel
    assert len(R.BN_CASES) == len(set(R.BN_CASES)) and set(R.BN_REGIMES) == {"moderate", "offset"}
