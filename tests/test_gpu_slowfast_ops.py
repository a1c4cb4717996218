"""Per-kernel parity of everything SlowFast R50 runs around its convolutions (csrc/slowfast.hip, the statistics reduction and the
accumulate form of csrc/conv3d.hip, and the block / fusion / stem orchestration of slowfast_engine.py at reduced width) against plain
fp64 torch on the CPU: autograd of torch.nn.functional, or tests/slowfast_ref.py.  Every test builds its own reference.  The exact
checks (max-pool, ingest, canaries, refusals) have no tolerance; every other gate is twice the worst case measured on an MI355X,
rounded up to one significant digit (the measured value is next to the gate), and none exceeds GRAD_TOL_UNIT."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from mintime_amd import lib as L, slowfast as S, slowfast_engine as E

from . import slowfast_ref as R
from .test_gpu_slowfast import CONV_TOL, _fm_from_ncdhw, _to_ncdhw
from .util import GRAD_TOL_UNIT, rel_err

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)

CANARY = 7.0
EPS = 1e-5
MARGIN, PUSH = 1e-3, 1e-2      # ReLU conditioning: no pre-activation within MARGIN of zero (those drawn there are moved by PUSH)

BN_FWD_TOL = 2e-7              # measured worst case: 6.3e-8 (C = 80, residual with its own scale / shift)
BN_FOLD_TOL = 2e-7             # measured worst case: 9.2e-8 (scale, rows 131372 in training)
BN_BWD_TOL = 5e-7              # measured worst case: 2.4e-7 (dgamma of the plain adjoint in training, rows 1030, C 8)
HEAD_TOL = 8e-7                # measured worst case: 3.6e-7 (logits, CT = 132, J = 1)
# the block, fusion and stem tests cannot keep interior pre-activations away from zero; no ReLU or arg-max flip shows at these seeds
BLOCK_TOL = 2e-6               # measured worst case: 7.5e-7 (projection bottleneck in training, norm_a weight gradient)
FUSION_TOL = 1e-6              # measured worst case: 4.5e-7 (training, convolution weight gradient)
STEM_TOL = 2e-6                # measured worst case: 8.2e-7 (forward output)
assert max(BN_BWD_TOL, BN_FOLD_TOL, HEAD_TOL, BLOCK_TOL, FUSION_TOL, STEM_TOL) <= GRAD_TOL_UNIT and BN_FWD_TOL <= CONV_TOL


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _d(t):
    return t.float().contiguous().to(dev)


def _slice(t, width, off, fill=None, g=None):
    """t ([rows, C], CPU) as the column slice [off, off + C) of a `width`-wide device tensor (the rest: `fill`, or noise)."""
    wide = torch.full((t.shape[0], width), float(fill)) if fill is not None else torch.randn(t.shape[0], width, generator=g)
    wide[:, off:off + t.shape[1]] = t.float()
    wide = wide.to(dev)
    return wide, wide[:, off:off + t.shape[1]]


def _outside_untouched(wide, off, C, fill=CANARY):
    keep = torch.ones(wide.shape[1], dtype=torch.bool)
    keep[off:off + C] = False
    return bool(torch.all(wide.cpu()[:, keep] == fill))


class _Holder(nn.Module):
    """One module of the network under the name `m`, so that E._Walk finds its parameters and BatchNorm modules by key."""

    def __init__(self, m):
        super().__init__()
        self.m = m


def _randomise(holder, seed):
    """Non-trivial BatchNorm affine parameters and running statistics; returns the fp64 CPU state dict of the reference."""
    g = _gen(seed)
    sd = holder.state_dict()
    for k, v in sd.items():
        if k.endswith("running_var"):
            v.copy_(torch.rand(v.shape, generator=g) * 0.5 + 0.75)
        elif k.endswith("running_mean"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif "norm" in k and k.endswith(".weight"):
            v.copy_(torch.rand(v.shape, generator=g) * 0.6 + 0.7)
        elif "norm" in k and k.endswith(".bias"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    return {k: v.detach().clone().double() if v.is_floating_point() else v.detach().clone() for k, v in holder.state_dict().items()}


def _walk(holder, training):
    holder.to(dev)
    names = [n for n, _ in holder.named_parameters()]
    return E._Walk(holder, names, [p for _, p in holder.named_parameters()], training)


def _ref_params(sd):
    return {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}


def _rows(x):
    """[N, C, T, H, W] -> [N*T*H*W, C]."""
    return x.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1])


def _worst(pairs):
    errs = {k: rel_err(got, want) for k, (got, want) in pairs.items()}
    k = max(errs, key=errs.get)
    return errs[k], k


# ---- 1. BatchNorm + ReLU + residual forward -----------------------------------------------------------------------------------

def _bn_relu_fwd(z, sc, sh, res, rsc, rsh, y, rows, Cn):
    L.check(L.get().mt_sf_bn_relu_fwd(L.ptr(z), z.stride(0), L.ptr(sc), L.ptr(sh), L.ptr(res), res.stride(0) if res is not None else 0,
                                      L.ptr(rsc), L.ptr(rsh), L.ptr(y), y.stride(0), rows, Cn, L.stream_ptr()), "mt_sf_bn_relu_fwd")


@pytest.mark.parametrize("mode", ["none", "identity", "affine"])
@pytest.mark.parametrize("Cn", [8, 80])
def test_bn_relu_residual_forward_pitched(Cn, mode):
    rows = 515
    g = _gen(100 + Cn)
    z = torch.randn(rows, Cn, generator=g)
    res = torch.randn(rows, Cn, generator=g)
    sc, sh = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g) * 0.3
    rsc, rsh = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g) * 0.3
    u = z.double() * sc.double() + sh.double()
    if mode == "identity":
        u = u + res.double()
    elif mode == "affine":
        u = u + (res.double() * rsc.double() + rsh.double())
    _, zs = _slice(z, Cn + 24, 8, g=g)
    _, rs = _slice(res, Cn + 12, 4, g=g)
    ywide, ys = _slice(torch.zeros(rows, Cn), Cn + 20, 12, fill=CANARY)
    ys.fill_(CANARY)
    _bn_relu_fwd(zs, _d(sc), _d(sh), rs if mode != "none" else None, _d(rsc) if mode == "affine" else None,
                 _d(rsh) if mode == "affine" else None, ys, rows, Cn)
    torch.cuda.synchronize()
    e = rel_err(ys, F.relu(u))
    print(f"bn_relu_fwd C={Cn} {mode}: {e:.2e}")
    assert e <= BN_FWD_TOL
    assert _outside_untouched(ywide, 12, Cn)


def test_bn_relu_forward_refusals_leave_the_output_alone():
    rows = 33
    g = _gen(3)
    z, res = _d(torch.randn(rows, 8, generator=g)), _d(torch.randn(rows, 8, generator=g))
    v = _d(torch.rand(8, generator=g) + 0.5)
    y = torch.full((rows, 8), CANARY, device=dev)
    with pytest.raises(L.MintimeHipError, match=r"\(-3\).*float4"):              # MT_ERR_UNSUPPORTED
        _bn_relu_fwd(z, v, v, None, None, None, y, rows, 6)
    torch.cuda.synchronize()
    assert torch.all(y == CANARY)
    with pytest.raises(L.MintimeHipError, match=r"\(-1\).*need res"):            # MT_ERR_ARG
        _bn_relu_fwd(z, v, v, None, v, v, y, rows, 8)
    torch.cuda.synchronize()
    assert torch.all(y == CANARY)
    _bn_relu_fwd(z, v, v, res, v, v, y, rows, 8)                                 # the same operands are accepted once res is there
    torch.cuda.synchronize()
    assert not torch.any(y == CANARY)


# ---- 2. BatchNorm (+ ReLU) adjoint ----------------------------------------------------------------------------------------------

class _Norm(nn.Module):
    def __init__(self, Cn):
        super().__init__()
        self.norm = nn.BatchNorm3d(Cn, eps=EPS, momentum=0.1)


def _fold64(z, gamma, beta, rm, rv, training):
    """fp64 (scale, shift) of the BatchNorm over the rows of z."""
    mean, var = (z.mean(0), z.var(0, unbiased=False)) if training else (rm, rv)
    scale = gamma / torch.sqrt(var + EPS)
    return scale, beta - mean * scale


def _bn_case(rows, Cn, mode, training, seed):
    """A conditioned BatchNorm(+ReLU) adjoint problem and its fp64 answer.  mode: "relu_bn" (the ReLU of this BatchNorm's own
    output), "mask" (the ReLU of output + residual, recorded as the block output) or "none" (no ReLU)."""
    g = _gen(seed)
    mod = _Norm(Cn)
    with torch.no_grad():
        mod.norm.weight.copy_(torch.rand(Cn, generator=g) * 0.6 + 0.7)
        mod.norm.bias.copy_(torch.randn(Cn, generator=g) * 0.2)
        mod.norm.running_mean.copy_(torch.randn(Cn, generator=g) * 0.2 + 0.3)
        mod.norm.running_var.copy_(torch.rand(Cn, generator=g) * 2.0 + 2.0)
    gamma, beta = mod.norm.weight.detach().double(), mod.norm.bias.detach().double()
    rm, rv = mod.norm.running_mean.double().clone(), mod.norm.running_var.double().clone()
    z = (torch.randn(rows, Cn, generator=g) * 1.7 + 0.3).double()
    res = torch.randn(rows, Cn, generator=g).double()
    if mode == "relu_bn":
        # the device decides the ReLU in fp32, the reference in fp64: keep every pre-activation out of the margin around zero
        # (moving z moves the batch statistics a little, hence the repeat)
        for _ in range(8):
            scale, shift = _fold64(z, gamma, beta, rm, rv, training)
            u = z * scale + shift
            near = u.abs() < MARGIN
            if not near.any():
                break
            z = torch.where(near, z + torch.where(u >= 0, PUSH, -PUSH) / scale, z).float().double()
    scale, shift = _fold64(z, gamma, beta, rm, rv, training)
    u = z * scale + shift
    m = None
    if mode == "mask":
        near = (u + res).abs() < MARGIN
        res = torch.where(near, res + torch.where(u + res >= 0, PUSH, -PUSH), res).float().double()
        u = u + res
        m = F.relu(u).float()                           # the recorded block output: positive exactly where u is
        assert bool(((m > 0) == (u > 0)).all())
    if mode != "none":
        assert not bool((u.abs() < MARGIN).any())
    gy = torch.randn(rows, Cn, generator=g).double()
    zr = z.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm_new, rv_new = rm.clone(), rv.clone()
    y = F.batch_norm(zr, rm_new, rv_new, gr, br, training, 0.1, EPS)
    if mode == "mask":
        y = y + res
    if mode != "none":
        y = F.relu(y)
    y.backward(gy)
    return dict(mod=mod, z=z, gy=gy, m=m, scale=scale, shift=shift, dz=zr.grad, dgamma=gr.grad, dbeta=br.grad, rm=rm, rv=rv,
                rm_new=rm_new, rv_new=rv_new)


def _bn_forward(c, training, rows):
    """bn_fwd on the device from the fp64 column sums it normally receives; returns (walk, BN record, z Fm)."""
    walk = _walk(c["mod"], training)
    zt = _d(c["z"])
    stats = torch.cat([c["z"].sum(0), (c["z"] ** 2).sum(0)]).to(dev) if training else None
    b = E.bn_fwd(walk, "norm", stats, rows)
    return walk, b, E.Fm(zt, 1, 1, 1, rows)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("mode", ["relu_bn", "mask", "none"])
@pytest.mark.parametrize("rows,Cn", [(1030, 8), (1030, 72), (131072 + 300, 8)])
def test_bn_relu_adjoint_matches_fp64_autograd(rows, Cn, mode, training):
    c = _bn_case(rows, Cn, mode, training, seed=rows % 1000 + Cn)
    walk, b, z = _bn_forward(c, training, rows)
    norm = c["mod"].norm
    e_fold, k_fold = _worst({"scale": (b.scale, c["scale"]), "shift": (b.shift, c["shift"]),
                             "running_mean": (norm.running_mean, c["rm_new"]), "running_var": (norm.running_var, c["rv_new"])})
    assert int(norm.num_batches_tracked) == (1 if training else 0)
    if not training:                                    # eval reads the running statistics and leaves them as they are
        assert torch.equal(norm.running_mean.cpu().double(), c["rm"]) and torch.equal(norm.running_var.cpu().double(), c["rv"])
    _, gs = _slice(c["gy"], Cn + 8, 4, g=_gen(1))
    mask = None
    if mode == "mask":
        _, ms = _slice(c["m"], Cn + 12, 8, g=_gen(2))
        mask = E.Fm(ms, 1, 1, 1, rows)
    dz = E.bn_bwd(walk, b, E.Fm(gs, 1, 1, 1, rows), z, relu_bn=b if mode == "relu_bn" else None, mask=mask)
    torch.cuda.synchronize()
    e, k = _worst({"dz": (dz.t, c["dz"]), "dgamma": (walk.grads["norm.weight"], c["dgamma"]),
                   "dbeta": (walk.grads["norm.bias"], c["dbeta"])})
    print(f"bn adjoint rows={rows} C={Cn} {mode} training={training}: fold {e_fold:.2e} ({k_fold}), adjoint {e:.2e} ({k})")
    assert e_fold <= BN_FOLD_TOL, (e_fold, k_fold)
    assert e <= BN_BWD_TOL, (e, k)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("form", ["accumulate", "in_place", "in_place_pitched"])
def test_bn_relu_adjoint_accumulate_and_in_place(form, training):
    rows, Cn = 1030, 72
    c = _bn_case(rows, Cn, "relu_bn", training, seed=5)
    walk, b, z = _bn_forward(c, training, rows)
    g = _gen(6)
    want = c["dz"]
    if form == "accumulate":
        old = torch.randn(rows, Cn, generator=g)
        wide, out = _slice(old, Cn + 8, 4, fill=CANARY)
        gfm = E.Fm(_d(c["gy"]), 1, 1, 1, rows)
        want = old.double() + want
    else:
        off = 4 if form == "in_place_pitched" else 0
        wide, out = _slice(c["gy"], Cn + 2 * off, off, fill=CANARY)
        gfm = E.Fm(out, 1, 1, 1, rows)                   # out is g, as block_bwd does with gb / ga
    dz = E.bn_bwd(walk, b, gfm, z, relu_bn=b, out=out, accumulate=form == "accumulate")
    torch.cuda.synchronize()
    assert dz.t.data_ptr() == out.data_ptr()
    e, k = _worst({"dz": (out, want), "dgamma": (walk.grads["norm.weight"], c["dgamma"]), "dbeta": (walk.grads["norm.bias"], c["dbeta"])})
    print(f"bn adjoint {form} training={training}: {e:.2e} ({k})")
    assert e <= BN_BWD_TOL, (e, k)
    assert _outside_untouched(wide, 4 if form != "in_place" else 0, Cn)
    # a second adjoint through the same walk adds to dgamma / dbeta
    E.bn_bwd(walk, b, E.Fm(_d(c["gy"]), 1, 1, 1, rows), z, relu_bn=b)
    torch.cuda.synchronize()
    assert rel_err(walk.grads["norm.weight"], 2 * c["dgamma"]) <= BN_BWD_TOL
    assert rel_err(walk.grads["norm.bias"], 2 * c["dbeta"]) <= BN_BWD_TOL


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("masked", [True, False])
def test_identity_shortcut_adjoint_is_exact(masked, accumulate):
    """block_bwd's call for the identity shortcut: no kabc, z, scale or shift; out (+)= g where the block output is positive."""
    rows, Cn = 1030, 72
    g = _gen(7)
    gy = torch.randn(rows, Cn, generator=g)
    y = F.relu(torch.randn(rows, Cn, generator=g))
    old = torch.randn(rows, Cn, generator=g)
    _, gs = _slice(gy, Cn + 8, 4, g=g)
    _, ys = _slice(y, Cn + 4, 4, g=g)
    wide, out = _slice(old, Cn + 12, 8, fill=CANARY)
    L.check(L.get().mt_sf_bn_relu_bwd_apply(L.ptr(gs), gs.stride(0), None, 0, None, None, L.ptr(ys) if masked else None,
                                            ys.stride(0) if masked else 0, None, L.ptr(out), out.stride(0), accumulate, rows, Cn,
                                            L.stream_ptr()), "mt_sf_bn_relu_bwd_apply")
    torch.cuda.synchronize()
    want = torch.where(y > 0, gy, torch.zeros(())) if masked else gy
    if accumulate:
        want = old + want                                # one fp32 addition: the same on both sides
    assert torch.equal(out.cpu(), want)
    assert _outside_untouched(wide, 8, Cn)


# ---- 3. stem max-pool ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [8, 5])
@pytest.mark.parametrize("H,W", [(7, 9), (8, 6), (1, 1)])
def test_stem_maxpool_forward_and_adjoint_bit_exact(H, W, Cn):
    NT = 3
    g = _gen(H * 10 + Cn)
    # dyadic operands: z * scale + shift is exact in fp32, so ties among positive values and among post-ReLU zeros are genuine
    z = torch.randint(-16, 17, (NT, H, W, Cn), generator=g).double() / 8
    scale = torch.tensor([0.5, 1.0, 2.0, 0.25])[torch.randint(0, 4, (Cn,), generator=g)].double()
    shift = torch.randint(-2, 3, (Cn,), generator=g).double() / 4
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dout = torch.randint(-16, 17, (NT, Ho, Wo, Cn), generator=g).double() / 8

    def ref(dt):
        x = F.relu(z.to(dt) * scale.to(dt) + shift.to(dt)).permute(3, 0, 1, 2)[None].detach().requires_grad_(True)
        o, idx = F.max_pool3d(x, (1, 3, 3), (1, 2, 2), (0, 1, 1), return_indices=True)
        o.backward(dout.to(dt).permute(3, 0, 1, 2)[None])
        arg = idx - (torch.arange(NT) * H * W)[None, None, :, None, None]
        return x.detach(), o.detach()[0].permute(1, 2, 3, 0), arg[0].permute(1, 2, 3, 0), x.grad[0].permute(1, 2, 3, 0)

    x64, o64, a64, d64 = ref(torch.float64)
    _, o32, a32, d32 = ref(torch.float32)
    assert torch.equal(o32.double(), o64) and torch.equal(a32, a64) and torch.equal(d32.double(), d64)      # the inputs are exact
    if H > 1:
        assert float((x64 == 0).double().mean()) > 0.3 and bool((o64 == 0).any())         # all-zero windows occur
    rows = NT * Ho * Wo
    owide, out = _slice(torch.zeros(rows, Cn), Cn + 7, 4, fill=CANARY)
    arg = torch.full((rows, Cn), -1, dtype=torch.int32, device=dev)
    lib = L.get()
    zt, sc, sh = _d(z.reshape(-1, Cn)), _d(scale), _d(shift)
    L.check(lib.mt_sf_maxpool_fwd(L.ptr(zt), L.ptr(sc), L.ptr(sh), L.ptr(out), out.stride(0), L.ptr(arg), NT, H, W, Cn, L.stream_ptr()),
            "mt_sf_maxpool_fwd")
    _, ds = _slice(dout.reshape(-1, Cn), Cn + 3, 2, g=g)
    din = torch.full((NT * H * W, Cn), CANARY, device=dev)
    L.check(lib.mt_sf_maxpool_bwd(L.ptr(ds), ds.stride(0), L.ptr(arg), L.ptr(din), NT, H, W, Cn, L.stream_ptr()), "mt_sf_maxpool_bwd")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), o32.reshape(-1, Cn))
    assert torch.equal(arg.cpu().long(), a64.reshape(-1, Cn))
    assert torch.equal(din.cpu(), d32.reshape(-1, Cn))
    assert _outside_untouched(owide, 4, Cn)


# ---- 4. head ------------------------------------------------------------------------------------------------------------------

HEAD_B = 2
HEAD_GRIDS = (((3, 4, 5), (2, 3, 3)), ((6, 4, 5), (5, 3, 3)))       # (feature grid, pool kernel) of the slow and the fast pathway
HEAD_P = (2, 2, 3)


def _head_case(Cs, Cf, J, with_mult, with_bias, seed):
    g = _gen(seed)
    B, CT = HEAD_B, Cs + Cf
    P = HEAD_P[0] * HEAD_P[1] * HEAD_P[2]
    feats = [torch.randn(B, Cn, *grid, generator=g).double() for Cn, (grid, _) in zip((Cs, Cf), HEAD_GRIDS)]
    w = (torch.randn(J, CT, generator=g) * 0.2).double()
    bias = (torch.randn(J, generator=g) * 0.5).double() if with_bias else None
    mult = ((torch.rand(B, CT, *HEAD_P, generator=g) >= 0.5).double() / 0.5) if with_mult else None
    gl = torch.randn(B, J, generator=g).double()
    fr = [f.clone().requires_grad_(True) for f in feats]
    wr = w.clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True) if with_bias else None
    pooled = torch.cat([F.avg_pool3d(f, k, stride=1) for f, (_, k) in zip(fr, HEAD_GRIDS)], 1)
    pooled.retain_grad()
    x = pooled * mult if with_mult else pooled
    y = F.linear(x.permute(0, 2, 3, 4, 1), wr, br).reshape(B, P, J).mean(1)
    y.backward(gl)
    rows3 = lambda t: t.detach().permute(0, 2, 3, 4, 1).reshape(B, P, CT)  # noqa: E731
    return dict(feats=feats, w=w, bias=bias, mult=rows3(mult) if with_mult else None, gl=gl, logits=y.detach(), dw=wr.grad,
                db=br.grad if with_bias else None, dpool=rows3(pooled.grad), dfeat=[f.grad for f in fr], P=P, CT=CT)


def _head_forward(c, Cs, Cf):
    lib = L.get()
    B, P, CT = HEAD_B, c["P"], c["CT"]
    mult = _d(c["mult"]) if c["mult"] is not None else None
    d = torch.full((B, P, CT), CANARY, device=dev)
    for f, Cn, (grid, k), coff in zip(c["feats"], (Cs, Cf), HEAD_GRIDS, (0, Cs)):
        _, fs = _slice(_rows(f), Cn + 8, 4, g=_gen(9))
        L.check(lib.mt_sf_head_pool(L.ptr(fs), fs.stride(0), L.ptr(mult), L.ptr(d), B, *grid, Cn, *k, coff, CT, L.stream_ptr()),
                "mt_sf_head_pool")
    return d, mult


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("with_mult", [True, False], ids=["mult", "nomult"])
@pytest.mark.parametrize("J", [1, 3])
@pytest.mark.parametrize("Cs,Cf", [(12, 8), (100, 32)])
def test_head_forward_and_backward_match_fp64_autograd(Cs, Cf, J, with_mult, with_bias):
    c = _head_case(Cs, Cf, J, with_mult, with_bias, seed=Cs + J)
    lib = L.get()
    B, P, CT = HEAD_B, c["P"], c["CT"]
    d, mult = _head_forward(c, Cs, Cf)
    w, bias, gl = _d(c["w"]), (_d(c["bias"]) if with_bias else None), _d(c["gl"])
    logits = torch.empty(B, J, device=dev)
    L.check(lib.mt_sf_head_proj(L.ptr(d), L.ptr(w), L.ptr(bias), L.ptr(logits), B, P, CT, J, L.stream_ptr()), "mt_sf_head_proj")
    g = _gen(10)
    dw0, db0 = torch.randn(J, CT, generator=g), torch.randn(J, generator=g)        # head_params accumulates: old + gradient
    dw, db = _d(dw0), (_d(db0) if with_bias else None)
    dpool = torch.empty(B, P, CT, device=dev)
    L.check(lib.mt_sf_head_bwd(L.ptr(gl), L.ptr(d), L.ptr(w), L.ptr(mult), L.ptr(dw), L.ptr(db), L.ptr(dpool), B, P, CT, J,
                               L.stream_ptr()), "mt_sf_head_bwd")
    pairs = {"logits": (logits, c["logits"]), "dW": (dw, dw0.double() + c["dw"]), "dpool": (dpool, c["dpool"])}
    if with_bias:
        pairs["db"] = (db, db0.double() + c["db"])
    wides = []
    for i, (f, Cn, (grid, k), coff) in enumerate(zip(c["feats"], (Cs, Cf), HEAD_GRIDS, (0, Cs))):
        wide, gs = _slice(torch.zeros(f.numel() // Cn, Cn), Cn + 12, 8, fill=CANARY)
        L.check(lib.mt_sf_head_dfeat(L.ptr(dpool), L.ptr(gs), gs.stride(0), B, *grid, Cn, *k, coff, CT, L.stream_ptr()), "mt_sf_head_dfeat")
        pairs[f"dfeat{i}"] = (gs, _rows(c["dfeat"][i]))
        wides.append((wide, Cn))
    torch.cuda.synchronize()
    e, k = _worst(pairs)
    print(f"head C=({Cs},{Cf}) J={J} mult={with_mult} bias={with_bias}: {e:.2e} ({k})")
    assert e <= HEAD_TOL, (e, k)
    assert all(_outside_untouched(wide, 8, Cn) for wide, Cn in wides)


@pytest.mark.parametrize("which", ["dw_only", "db_only"])
def test_head_parameter_gradients_one_at_a_time(which):
    Cs, Cf, J = 12, 8, 3
    c = _head_case(Cs, Cf, J, True, True, seed=11)
    B, P, CT = HEAD_B, c["P"], c["CT"]
    d, mult = _head_forward(c, Cs, Cf)
    g = _gen(12)
    dw0, db0 = torch.randn(J, CT, generator=g), torch.randn(J, generator=g)
    dw, db, gl, w = _d(dw0), _d(db0), _d(c["gl"]), _d(c["w"])
    L.check(L.get().mt_sf_head_bwd(L.ptr(gl), L.ptr(d), L.ptr(w), L.ptr(mult), L.ptr(dw) if which == "dw_only" else None,
                                   L.ptr(db) if which == "db_only" else None, None, B, P, CT, J, L.stream_ptr()), "mt_sf_head_bwd")
    torch.cuda.synchronize()
    e = rel_err(dw, dw0.double() + c["dw"]) if which == "dw_only" else rel_err(db, db0.double() + c["db"])
    print(f"head {which}: {e:.2e}")
    assert e <= HEAD_TOL
    assert torch.equal(db.cpu(), db0) if which == "dw_only" else torch.equal(dw.cpu(), dw0)


# ---- 5. ingest ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("layout", ["bfhwc", "bcfhw", "bcfhw_view"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_ingest_small_is_exact(dtype, layout, normalize):
    B, Fr, H, W = 2, 8, 5, 7
    g = _gen(13)
    v = torch.randint(0, 256, (B, Fr, H, W, 3), generator=g, dtype=torch.uint8)
    v = v if dtype == torch.uint8 else v.float() + torch.rand(v.shape, generator=g)
    fidx, split = [3, 0, 0, 7, 5, 2, 7], 3                      # repeats, not monotone; both outputs are written
    src = v.to(dev)
    if layout == "bcfhw":
        src = src.permute(0, 4, 1, 2, 3).contiguous()
    elif layout == "bcfhw_view":
        src = src.permute(0, 4, 1, 2, 3)
    out, out2 = S.ingest(src, fidx, normalize, "bfhwc" if layout == "bfhwc" else "bcfhw", split=split)
    torch.cuda.synchronize()
    x = v[:, fidx].float()
    if normalize:
        x = (x / torch.full_like(x, 255.0) - torch.full_like(x, 0.45)) / torch.full_like(x, 0.225)     # the reference's fp32 arithmetic
    got = torch.cat([out, out2], 1).cpu()
    assert out.shape == (B, split, H, W, 4) and out2.shape == (B, len(fidx) - split, H, W, 4)
    assert torch.equal(got[..., :3], x)
    assert torch.all(got[..., 3] == 0)


# ---- 6. two-level statistics reduction and forward accumulate of conv3d.hip ------------------------------------------------------

def test_conv_statistics_over_more_than_512_row_blocks():
    """33792 output rows = 528 blocks of 64 rows: the column sums take the second reduction level, with a partial last chunk."""
    g = _gen(14)
    cin, cout = 16, 8
    x = torch.randn(1, cin, 4, 96, 88, generator=g).double()
    w = (torch.randn(cout, cin, 1, 1, 1, generator=g) / cin ** 0.5).double()
    sc, sh = (torch.rand(cin, generator=g) + 0.5).double(), (torch.randn(cin, generator=g) * 0.3).double()
    y_ref = F.conv3d(F.relu(x * sc[None, :, None, None, None] + sh[None, :, None, None, None]), w)
    conv = E.Conv("w", (1, 1, 1), (1, 1, 1), (0, 0, 0))
    z, st = E.conv_fwd(_fm_from_ncdhw(x), _d(w), conv, (_d(sc), _d(sh)))
    torch.cuda.synchronize()
    assert z.rows == 33792 and st.shape == (2 * cout,)
    e_fwd = rel_err(_to_ncdhw(z), y_ref)
    e_s = rel_err(st[:cout], y_ref.sum((0, 2, 3, 4)))
    e_q = rel_err(st[cout:], (y_ref ** 2).sum((0, 2, 3, 4)))
    print(f"conv two-level stats: fwd {e_fwd:.2e} sum {e_s:.2e} sumsq {e_q:.2e}")
    assert e_fwd <= CONV_TOL and e_s <= CONV_TOL and e_q <= CONV_TOL, (e_fwd, e_s, e_q)


def test_conv_forward_accumulate_and_its_refusal_with_statistics():
    g = _gen(15)
    cin, cout = 16, 24
    k, s, p = (1, 3, 3), (1, 2, 2), (0, 1, 1)
    x = torch.randn(1, cin, 2, 7, 9, generator=g).double()
    w = (torch.randn(cout, cin, *k, generator=g) / (cin * 9) ** 0.5).double()
    xf = _fm_from_ncdhw(x)
    d, (To, Ho, Wo) = E._desc(xf, k, s, p, cout, cout)
    rows = To * Ho * Wo
    y0 = torch.randn(rows, cout, generator=g)
    y = _d(y0)
    wp = E._pack_w(_d(w), cin)
    lib = L.get()
    L.check(lib.mt_conv3d_fwd(C.byref(d), L.ptr(xf.t), None, None, L.ptr(wp), L.ptr(y), 1, None, None, L.stream_ptr()), "mt_conv3d_fwd")
    torch.cuda.synchronize()
    want = y0.double() + _rows(F.conv3d(x, w, stride=s, padding=p))
    e = rel_err(y, want)
    print(f"conv fwd accumulate: {e:.2e}")
    assert e <= CONV_TOL
    before = y.clone()
    part = torch.empty(int(lib.mt_conv3d_part_floats(C.byref(d))), device=dev)
    st = torch.full((2 * cout,), CANARY, dtype=torch.float64, device=dev)
    with pytest.raises(L.MintimeHipError, match=r"\(-1\).*accumulated"):
        L.check(lib.mt_conv3d_fwd(C.byref(d), L.ptr(xf.t), None, None, L.ptr(wp), L.ptr(y), 1, L.ptr(part), L.ptr(st), L.stream_ptr()),
                "mt_conv3d_fwd")
    torch.cuda.synchronize()
    assert torch.equal(y, before) and torch.all(st == CANARY)


# ---- 7. block, fusion and stem orchestration at reduced width ----------------------------------------------------------------------

def _block_check(blk, cin, kt, stride, first, N, T, H, W, training, seed, with_pro, pitched_g, canary_out):
    g = _gen(seed)
    holder = _Holder(blk)
    sd = _randomise(holder, seed)
    before = {k: v.clone() for k, v in sd.items()}
    x = torch.randn(N, cin, T, H, W, generator=g)
    pro = None
    if with_pro:
        sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
        pro = (_d(sc), _d(sh))
        xin = F.relu(x.double() * sc.double()[None, :, None, None, None] + sh.double()[None, :, None, None, None])
    else:
        x = F.relu(x)                                    # a block input without a prologue is a block output
        xin = x.double()
    xin = xin.detach().requires_grad_(True)
    params = _ref_params(sd)
    y_ref = R._block(xin, sd, "m", kt, stride, first, training)
    gy = torch.randn(y_ref.shape, generator=g).double()
    y_ref.backward(gy)
    walk = _walk(holder, training)
    cout = y_ref.shape[1]
    rows_out = y_ref.numel() // cout
    wide, out = (None, None)
    if canary_out:
        wide, out = _slice(torch.zeros(rows_out, cout), cout + 16, 0, fill=CANARY)
    y, rec = E.block_fwd(walk, "m", _fm_from_ncdhw(x), pro, kt, stride, first, out=out)
    gyt = _slice(_rows(gy), cout + 8, 4, g=g)[1] if pitched_g else _d(_rows(gy))
    gx = E.block_bwd(walk, rec, E.Fm(gyt, y.N, y.T, y.H, y.W))
    torch.cuda.synchronize()
    assert (y.N, y.T, y.H, y.W) == (N, T, (H - 1) // stride + 1, (W - 1) // stride + 1)
    pairs = {"y": (y.t, _rows(y_ref.detach())), "gx": (gx, _rows(xin.grad))}
    assert set(walk.grads) == set(params)
    for k, p in params.items():
        pairs[k] = (walk.grads[k], p.grad)
    buf = dict(holder.named_buffers())
    for k, v in sd.items():
        if "running" in k:
            pairs[k] = (buf[k], v.detach())
        elif k.endswith("num_batches_tracked"):
            assert int(buf[k]) == (1 if training else 0)
    if not training:
        assert all(torch.equal(buf[k].cpu().double(), before[k]) for k in sd if "running" in k)
    if canary_out:
        assert y.t.data_ptr() == out.data_ptr() and _outside_untouched(wide, 0, cout)
    return _worst(pairs)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_projection_bottleneck_forward_and_backward(training):
    torch.manual_seed(20)
    e, k = _block_check(S._ResBlock(32, 16, 64, 3, 2), 32, 3, 2, True, 2, 4, 18, 14, training, seed=21, with_pro=True, pitched_g=True,
                        canary_out=False)
    print(f"projection bottleneck training={training}: {e:.2e} ({k})")
    assert e <= BLOCK_TOL, (e, k)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_identity_bottleneck_forward_and_backward(training):
    torch.manual_seed(22)
    e, k = _block_check(S._ResBlock(64, 16, 64, 1, 1), 64, 1, 1, False, 2, 4, 9, 7, training, seed=23, with_pro=False, pitched_g=False,
                        canary_out=True)
    print(f"identity bottleneck training={training}: {e:.2e} ({k})")
    assert e <= BLOCK_TOL, (e, k)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_fusion_forward_and_backward(training):
    torch.manual_seed(24)
    g = _gen(25)
    cf, cs = 8, 16
    holder = _Holder(S._Fusion(cf))
    sd = _randomise(holder, 25)
    N, T, H, W = 2, 16, 6, 5
    xf = torch.randn(N, cf, T, H, W, generator=g).double()
    xr = xf.clone().requires_grad_(True)
    params = _ref_params(sd)
    rm, rv = sd["m.norm.running_mean"].clone(), sd["m.norm.running_var"].clone()
    xs = torch.zeros(N, cs, T // 4, H, W, dtype=torch.float64)
    tail = R._fusion(xs, xr, sd, "m", training)[:, cs:]
    gt = torch.randn(tail.shape, generator=g).double()
    tail.backward(gt)
    f_raw = F.conv3d(xf, sd["m.conv_fast_to_slow.weight"].detach(), stride=(4, 1, 1), padding=(3, 0, 0))
    scale, shift = _fold64(_rows(f_raw), sd["m.norm.weight"].detach(), sd["m.norm.bias"].detach(), rm, rv, training)
    walk = _walk(holder, training)
    rows = N * (T // 4) * H * W
    cat = torch.full((rows, cs + 2 * cf), CANARY, device=dev)
    pro, rec = E._fusion_fwd(walk, "m", _fm_from_ncdhw(xf), cat, cs)
    gcat = torch.cat([torch.randn(rows, cs, generator=g), _rows(gt).float()], 1).to(dev)
    gx0 = torch.randn(N * T * H * W, cf, generator=g)
    gxf = _d(gx0)
    E._fusion_bwd(walk, rec, gcat, cs, gxf)
    torch.cuda.synchronize()
    assert torch.all(pro[0][:cs] == 1) and torch.all(pro[1][:cs] == 0)
    assert torch.all(cat[:, :cs] == CANARY)
    assert set(walk.grads) == set(params)
    buf = dict(holder.named_buffers())
    pairs = {"raw": (cat[:, cs:], _rows(f_raw)), "scale": (pro[0][cs:], scale), "shift": (pro[1][cs:], shift),
             "gxf": (gxf, gx0.double() + _rows(xr.grad)), "running_mean": (buf["m.norm.running_mean"], sd["m.norm.running_mean"]),
             "running_var": (buf["m.norm.running_var"], sd["m.norm.running_var"])}
    pairs.update({k: (walk.grads[k], p.grad) for k, p in params.items()})
    e, k = _worst(pairs)
    print(f"fusion training={training}: {e:.2e} ({k})")
    assert e <= FUSION_TOL, (e, k)


def test_stem_forward_and_backward_at_odd_sizes():
    torch.manual_seed(26)
    g = _gen(27)
    holder = _Holder(S._Stem(8, 5))
    sd = _randomise(holder, 27)
    x = torch.randn(1, 3, 8, 22, 18, generator=g).double()
    params = _ref_params(sd)
    conv = F.conv3d(x, sd["m.conv.weight"], stride=(1, 2, 2), padding=(2, 3, 3))
    y_ref = F.max_pool3d(R._bn(conv, sd, "m.norm", True), (1, 3, 3), (1, 2, 2), (0, 1, 1))
    assert conv.shape[2:] == (8, 11, 9) and y_ref.shape[2:] == (8, 6, 5)
    gp = torch.randn(y_ref.shape, generator=g).double()
    y_ref.backward(gp)
    walk = _walk(holder, True)
    y, rec = E._stem_fwd(walk, "m", _fm_from_ncdhw(x, 4), 5, None)
    _, gs = _slice(_rows(gp), 8 + 8, 4, g=g)
    E._stem_bwd(walk, rec, E.Fm(gs, y.N, y.T, y.H, y.W))
    torch.cuda.synchronize()
    assert (y.T, y.H, y.W) == (8, 6, 5) and set(walk.grads) == set(params)
    buf = dict(holder.named_buffers())
    pairs = {"y": (y.t, _rows(y_ref.detach())), "running_mean": (buf["m.norm.running_mean"], sd["m.norm.running_mean"]),
             "running_var": (buf["m.norm.running_var"], sd["m.norm.running_var"])}
    pairs.update({k: (walk.grads[k], p.grad) for k, p in params.items()})
    e, k = _worst(pairs)
    print(f"stem: {e:.2e} ({k})")
    assert e <= STEM_TOL, (e, k)
