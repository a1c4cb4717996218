"""tests/effnet_ops_ref.py against torch autograd of the composed fp64 forward (CPU): the references of tests/test_gpu_effnet_ops.py
are the operations themselves, not a transcription of the kernels.  Everything is fp64, so the bounds are rounding of fp64 sums."""
import pytest
import torch
import torch.nn.functional as Fn

from . import effnet_ops_ref as R
from .util import rel_err

TOL = 1e-12      # fp64: ~1e3-term sums of O(1) values in two different orders differ by ~1e-14 relative


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _ru(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64) + 0.5


@pytest.mark.parametrize("k,s,H,W,kind", [(3, 1, 9, 6, 1), (3, 2, 8, 10, 2), (5, 1, 7, 11, 0), (5, 2, 10, 6, 1), (3, 2, 7, 9, 1),
                                          (5, 2, 9, 5, 2)])
def test_depthwise_reference_is_the_adjoint_of_conv2d(k, s, H, W, kind):
    """du_in, dW and the two sums of R.dw_bwd against autograd through conv2d o act o affine with the TF-SAME padding written out
    here, res_pre / res_post added as gradients of other consumers of the activated / the raw tensor; R.dw_fwd against the same."""
    N, C = 2, 8
    g = _g(100 * k + 10 * s + H)
    Ho, ph0, ph1 = R.same_pad(H, k, s)
    Wo, pw0, pw1 = R.same_pad(W, k, s)
    assert Ho == (H + s - 1) // s and ph0 + ph1 == max((Ho - 1) * s + k - H, 0) and ph0 == (ph0 + ph1) // 2
    zin = _rn(g, N * H * W, C).requires_grad_(True)
    w = _rn(g, C, 1, k, k).requires_grad_(True)
    scale, shift = _ru(g, C), _rn(g, C)
    du, z = _rn(g, N * Ho * Wo, C), _rn(g, N * Ho * Wo, C)
    kabc = _rn(g, 3, C)
    mi = torch.stack([_rn(g, C), _ru(g, C)])
    res_pre, res_post = _rn(g, N * H * W, C), _rn(g, N * H * W, C)
    u = zin * scale + shift
    a = R.act(u, kind)
    a_img = Fn.pad(a.reshape(N, H, W, C).permute(0, 3, 1, 2), (pw0, pw1, ph0, ph1))
    out = Fn.conv2d(a_img, w, stride=s, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
    zout, s_sum, s_sq = R.dw_fwd(zin.detach(), scale, shift, w.detach(), N, H, W, k, s, kind)
    assert rel_err(zout, out) <= TOL and rel_err(s_sum, out.sum(0)) <= TOL and rel_err(s_sq, (out * out).sum(0)) <= TOL
    dz = kabc[0] * du + kabc[1] * z + kabc[2]
    # the loss whose gradient is (g + res_pre) act'(u) + res_post with respect to zin / scale ... and dW with respect to w
    g_zin0 = torch.autograd.grad((out * dz).sum(), zin, retain_graph=True)[0]
    g_zin, g_w = torch.autograd.grad((out * dz).sum() + (a * res_pre).sum() + (u * res_post).sum(), (zin, w))
    for rp, rq in ((res_pre, res_post), (None, None)):
        du_in, s1, s2, dw = R.dw_bwd(du, z, kabc, w.detach(), zin.detach(), scale, shift, mi, N, H, W, k, s, kind, rp, rq)
        ref_in = (g_zin0 if rp is None else g_zin) / scale             # d/du = (d/dzin) / scale
        assert rel_err(du_in, ref_in) <= TOL
        assert rel_err(dw, g_w) <= TOL
        assert rel_err(s1, ref_in.sum(0)) <= TOL
        assert rel_err(s2, (ref_in * (zin.detach() - mi[0]) * mi[1]).sum(0)) <= TOL
    assert R.dw_bwd(du, z, kabc, w.detach(), zin.detach(), scale, shift, None, N, H, W, k, s, kind)[2] is None


def test_half_resolution_residual_sits_at_the_even_positions():
    N, H, W, C = 2, 5, 4, 3
    res = _rn(_g(1), N * 3 * 2, C)
    full = R.half_to_full(res, N, H, W).reshape(N, H, W, C)
    assert torch.equal(full[:, ::2, ::2].reshape(-1, C), res)
    assert float(full[:, 1::2].abs().sum()) == 0.0 and float(full[:, :, 1::2].abs().sum()) == 0.0


@pytest.mark.parametrize("training", [True, False])
def test_batchnorm_references_against_torch_batchnorm(training):
    """R.bn_finalize against nn.BatchNorm2d (scale / shift through its output, the running statistics after one step);
    dz = ka du + kb z + kc, dgamma and dbeta of R.bn_bwd_finalize against autograd of F.batch_norm."""
    N, H, W, C = 3, 5, 4, 6
    g = _g(7 + training)
    eps, momentum = 1e-3, 0.01
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(_ru(g, C)); bn.bias.copy_(_rn(g, C)); bn.running_mean.copy_(_rn(g, C)); bn.running_var.copy_(_ru(g, C))
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn.train(training)
    z = (_rn(g, N * H * W, C) * 2 + 1).requires_grad_(True)
    y = bn(R.nchw(z, N, H, W))
    count = N * H * W
    zd = z.detach()
    f = R.bn_finalize(zd.sum(0), (zd * zd).sum(0), count, bn.weight.detach(), bn.bias.detach(), rm0, rv0, eps, momentum, training)
    assert rel_err(zd * f["scale"] + f["shift"], R.nhwc_rows(y)) <= TOL
    assert rel_err(f["running_mean"], bn.running_mean) <= TOL and rel_err(f["running_var"], bn.running_var) <= TOL
    if not training:
        assert torch.equal(f["running_mean"], rm0) and torch.equal(f["running_var"], rv0)
    du = _rn(g, count, C)
    dz_ref, dgamma, dbeta = torch.autograd.grad(y, (z, bn.weight, bn.bias), R.nchw(du, N, H, W))
    mi = torch.stack([f["mean"], f["invstd"]])
    s1, s2 = du.sum(0), (du * (zd - mi[0]) * mi[1]).sum(0)
    kabc, add_gamma, add_beta = R.bn_bwd_finalize(s1, s2, count, bn.weight.detach(), mi, training)
    assert rel_err(kabc[0] * du + kabc[1] * zd + kabc[2], dz_ref) <= TOL
    assert rel_err(add_gamma, dgamma) <= TOL and rel_err(add_beta, dbeta) <= TOL
    if not training:
        assert float(kabc[1:].abs().sum()) == 0.0


def test_batchnorm_finalize_count_one_and_clamp():
    """count = 1: the running variance takes the biased value (no division by zero); a negative Q / count - m^2 is clamped."""
    one = torch.ones(2, dtype=torch.float64)
    f = R.bn_finalize(3 * one, 9 * one - torch.tensor([0.0, 1e-9]), 1, one, 0 * one, 0 * one, one, 1e-3, 0.1, True)
    assert torch.isfinite(f["running_var"]).all() and float(f["running_var"][1]) == 0.9
    assert float(f["invstd"][1]) == 1 / 1e-3 ** 0.5 and float(f["mean"][1]) == 3.0


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("with_gate,with_rowscale", [(True, True), (False, False), (True, False)])
def test_activation_adjoint_reference_against_autograd(kind, with_gate, with_rowscale):
    """R.bn_act_bwd: the gradient of y = act(z scale + shift) consumed as gate * y (din), through its mean over hw (dpool) and
    scaled per image (rowscale) -- autograd of exactly that composition."""
    N, hw, C = 3, 7, 4
    g = _g(40 + kind)
    z = _rn(g, N * hw, C).requires_grad_(True)
    scale, shift = _ru(g, C), _rn(g, C)
    din, gate, dpool, rs = _rn(g, N * hw, C), _ru(g, N, C), _rn(g, N, C), _ru(g, N)
    mi = torch.stack([_rn(g, C), _ru(g, C)])
    a = R.act(z * scale + shift, kind)
    n = torch.arange(N * hw) // hw
    r = rs[n].unsqueeze(1) if with_rowscale else 1.0
    if with_gate:
        loss = (a * gate[n] * din * r).sum() + ((a * r).reshape(N, hw, C).mean(1) * dpool).sum()
    else:
        loss = (a * din * r).sum()
    ref = torch.autograd.grad(loss, z)[0] / scale
    du, s1, s2 = R.bn_act_bwd(din, z.detach(), scale, shift, mi, gate if with_gate else None, dpool if with_gate else None,
                              rs if with_rowscale else None, hw, kind)
    assert rel_err(du, ref) <= TOL and rel_err(s1, ref.sum(0)) <= TOL
    assert rel_err(s2, (ref * (z.detach() - mi[0]) * mi[1]).sum(0)) <= TOL
    y = R.bn_act_fwd(z.detach(), scale, shift, din, kind, rs, hw)
    assert rel_err(y, (a * rs[n].unsqueeze(1) + din).detach()) <= TOL


def test_squeeze_excite_references_against_autograd():
    """R.se_fwd is the SE branch; R.se_bwd's dgate, dpooled and four weight gradients are autograd's of gated = a * gate[n]."""
    N, HW, C, CS = 3, 6, 8, 5
    g = _g(5)
    z = _rn(g, N * HW, C)
    scale, shift = _ru(g, C), _rn(g, C)
    w1, b1, w2, b2 = (t.requires_grad_(True) for t in (_rn(g, CS, C), _rn(g, CS), _rn(g, C, CS), _rn(g, C)))
    da = _rn(g, N * HW, C)
    a = R.act(z * scale + shift, 1)
    pooled = a.reshape(N, HW, C).mean(1).requires_grad_(True)
    hidden = Fn.linear(pooled, w1, b1)
    gate = torch.sigmoid(Fn.linear(Fn.silu(hidden), w2, b2))
    p, h, gt = R.se_fwd(z, scale, shift, w1.detach(), b1.detach(), w2.detach(), b2.detach(), N, HW)
    assert rel_err(p, pooled) <= TOL and rel_err(h, hidden) <= TOL and rel_err(gt, gate) <= TOL
    n = torch.arange(N * HW) // HW
    gate.retain_grad()
    (a * gate[n] * da).sum().backward()
    r = R.se_bwd(da, z, scale, shift, gt, h, p, w1.detach(), w2.detach(), N, HW)
    for name, ref in (("dgate", gate.grad), ("dpooled", pooled.grad), ("dw1", w1.grad), ("db1", b1.grad), ("dw2", w2.grad),
                      ("db2", b2.grad)):
        assert rel_err(r[name], ref) <= TOL, name
    r2 = R.se_bwd(None, None, None, None, gt, h, p, w1.detach(), w2.detach(), N, HW, dgate=r["dgate"])
    assert all(torch.equal(r[k], r2[k]) for k in r)


@pytest.mark.parametrize("H,W", [(8, 12), (9, 13), (6, 5)])
def test_stem_weight_gradient_reference_against_autograd(H, W):
    N = 2
    g = _g(H)
    Ho, ph0, ph1 = R.same_pad(H, 3, 2)
    Wo, pw0, pw1 = R.same_pad(W, 3, 2)
    x = _rn(g, N, H, W, 3)
    w = _rn(g, 32, 3, 3, 3).requires_grad_(True)
    du, z, kabc = _rn(g, N * Ho * Wo, 32), _rn(g, N * Ho * Wo, 32), _rn(g, 3, 32)
    out = Fn.conv2d(Fn.pad(x.permute(0, 3, 1, 2), (pw0, pw1, ph0, ph1)), w, stride=2)
    assert out.shape[2:] == (Ho, Wo)
    ref = torch.autograd.grad((R.nhwc_rows(out) * (kabc[0] * du + kabc[1] * z + kabc[2])).sum(), w)[0]
    assert rel_err(R.stem_wgrad(du, z, kabc, x, N, H, W), ref) <= TOL


def test_weight_pack_reference_is_the_im2col_operand():
    """Row co of the packed weight times the im2col patch (kh, kw, ci) is the convolution; unpack inverts pack and ignores padding."""
    Co, Ci, k, ld = 5, 3, 3, 28
    g = _g(9)
    w, x = _rn(g, Co, Ci, k, k), _rn(g, 1, Ci, k, k)
    wp = R.conv_weight_pack(w, ld)
    patch = x[0].permute(1, 2, 0).reshape(-1)
    assert rel_err(wp[:, :k * k * Ci] @ patch, Fn.conv2d(x, w).reshape(-1)) <= TOL
    assert float(wp[:, k * k * Ci:].abs().sum()) == 0.0
    wp[:, k * k * Ci:] = 7.0
    assert torch.equal(R.conv_weight_unpack(wp, Co, Ci, k), w)
