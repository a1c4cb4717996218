"""Plain torch definitions of the frame extractors' non-GEMM operations (csrc/effnet_fwd.hip, csrc/effnet_bwd.hip, csrc/xception.hip),
the reference side of tests/test_gpu_effnet_ops.py.  Every function computes in the dtype of its inputs: float64 is the reference,
float32 the yardstick.  Tensors are NHWC rows, [N*H*W, C]; weights are in torch layout.  Backward functions are written out as the
adjoints they are (no autograd); tests/test_effnet_ops_ref_host.py ties each one to torch autograd of the composed forward."""
import torch
import torch.nn.functional as Fn


def act(u, kind):
    """kind 0 none, 1 swish, 2 relu."""
    if kind == 1:
        return u * torch.sigmoid(u)
    if kind == 2:
        return torch.clamp_min(u, 0)
    return u


def dact(u, kind):
    if kind == 1:
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    if kind == 2:
        return (u > 0).to(u.dtype)
    return torch.ones_like(u)


def same_pad(size, k, s):
    """TF-SAME along one axis: (output size, pad before, pad after)."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2, total - total // 2


def nchw(rows, N, H, W):
    return rows.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def nhwc_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _padded_act(zin, scale, shift, N, H, W, k, s, kind):
    (Ho, ph0, ph1), (Wo, pw0, pw1) = same_pad(H, k, s), same_pad(W, k, s)
    a = nchw(act(zin * scale + shift, kind), N, H, W)
    return Fn.pad(a, (pw0, pw1, ph0, ph1)), Ho, Wo, ph0, pw0


def dw_fwd(zin, scale, shift, w, N, H, W, k, s, kind):
    """zout [N*Ho*Wo, C], sum zout, sum zout^2 (per channel)."""
    a_pad, _, _, _, _ = _padded_act(zin, scale, shift, N, H, W, k, s, kind)
    zout = nhwc_rows(Fn.conv2d(a_pad, w, stride=s, groups=w.shape[0]))
    return zout, zout.sum(0), (zout * zout).sum(0)


def half_to_full(res, N, H, W):
    """A residual given at the even (ih, iw) only, [N, ceil(H/2), ceil(W/2), C] rows -> full resolution, zero elsewhere."""
    C = res.shape[-1]
    full = torch.zeros(N, H, W, C, dtype=res.dtype)
    full[:, ::2, ::2] = res.reshape(N, (H + 1) // 2, (W + 1) // 2, C)
    return full.reshape(-1, C)


def dw_bwd(du, z, kabc, w, zin, scale_in, shift_in, mean_invstd_in, N, H, W, k, s, kind, res_pre=None, res_post=None):
    """du_in [N*H*W, C], S1 = sum du_in, S2 = sum du_in * xhat (None without mean_invstd_in), dW [C, 1, k, k]."""
    C = w.shape[0]
    a_pad, Ho, Wo, ph0, pw0 = _padded_act(zin, scale_in, shift_in, N, H, W, k, s, kind)
    dz = nchw(kabc[0] * du + kabc[1] * z + kabc[2], N, Ho, Wo)
    # adjoint with respect to the padded input: every output scatters its k x k taps; the padding is then cut off
    g_pad = torch.zeros_like(a_pad)
    dw = torch.zeros_like(w)
    for kh in range(k):
        for kw in range(k):
            win = (slice(None), slice(None), slice(kh, kh + (Ho - 1) * s + 1, s), slice(kw, kw + (Wo - 1) * s + 1, s))
            g_pad[win] += dz * w[:, 0, kh, kw].reshape(1, C, 1, 1)
            dw[:, 0, kh, kw] = (dz * a_pad[win]).sum((0, 2, 3))
    g = nhwc_rows(g_pad[:, :, ph0:ph0 + H, pw0:pw0 + W])
    if res_pre is not None:
        g = g + res_pre
    du_in = g * dact(zin * scale_in + shift_in, kind)
    if res_post is not None:
        du_in = du_in + res_post
    s2 = None
    if mean_invstd_in is not None:
        s2 = (du_in * (zin - mean_invstd_in[0]) * mean_invstd_in[1]).sum(0)
    return du_in, du_in.sum(0), s2, dw


def bn_finalize(S, Q, count, gamma, beta, running_mean, running_var, eps, momentum, training):
    """nn.BatchNorm2d's bookkeeping from the sums: dict of scale, shift, mean, invstd, running_mean, running_var."""
    if training:
        m = S / count
        v = torch.clamp_min(Q / count - m * m, 0)
        if running_mean is not None:
            unbiased = v * count / (count - 1) if count > 1 else v
            running_mean = (1 - momentum) * running_mean + momentum * m
            running_var = (1 - momentum) * running_var + momentum * unbiased
    else:
        m, v = running_mean, running_var
    invstd = 1 / torch.sqrt(v + eps)
    scale = gamma * invstd
    return {"scale": scale, "shift": beta - m * scale, "mean": m, "invstd": invstd, "running_mean": running_mean,
            "running_var": running_var}


def bn_bwd_finalize(S1, S2, count, gamma, mean_invstd, training):
    """kabc [3, C] with dz = ka du + kb z + kc, and what dgamma / dbeta receive."""
    mean, invstd = mean_invstd[0], mean_invstd[1]
    ka = gamma * invstd
    kb, kc = torch.zeros_like(ka), torch.zeros_like(ka)
    if training:
        kb = -ka * (S2 / count) * invstd
        kc = ka * (S2 / count) * invstd * mean - ka * S1 / count
    return torch.stack([ka, kb, kc]), S2, S1


def bn_act_fwd(z, scale, shift, res, kind, rowscale, rows_per_group):
    y = act(z * scale + shift, kind)
    if rowscale is not None:
        y = y * rowscale[torch.arange(z.shape[0]) // rows_per_group].unsqueeze(1)
    return y if res is None else y + res


def bn_act_bwd(din, z, scale, shift, mean_invstd, gate, dpool, rowscale, hw, kind):
    """du [rows, C], S1 = sum du, S2 = sum du * xhat."""
    n = torch.arange(z.shape[0]) // hw
    d = din
    if gate is not None:
        d = d * gate[n] + dpool[n] / hw
    if rowscale is not None:
        d = d * rowscale[n].unsqueeze(1)
    du = d * dact(z * scale + shift, kind)
    return du, du.sum(0), (du * (z - mean_invstd[0]) * mean_invstd[1]).sum(0)


def se_fwd(z, scale, shift, w1, b1, w2, b2, N, HW):
    """pooled [N, C], hidden [N, CS] (the pre-activation), gate [N, C]."""
    pooled = act(z * scale + shift, 1).reshape(N, HW, -1).mean(1)
    hidden = pooled @ w1.t() + b1
    gate = torch.sigmoid(act(hidden, 1) @ w2.t() + b2)
    return pooled, hidden, gate


def se_bwd(da, z, scale, shift, gate, hidden, pooled, w1, w2, N, HW, dgate=None):
    """The squeeze-excite adjoint; da = the gradient of the gated tensor.  With dgate given, da / z / scale / shift are not used."""
    if dgate is None:
        dgate = (da * act(z * scale + shift, 1)).reshape(N, HW, -1).sum(1)
    dpre2 = dgate * gate * (1 - gate)
    dhid = (dpre2 @ w2) * dact(hidden, 1)
    return {"dgate": dgate, "dpre2": dpre2, "dhid": dhid, "dpooled": dhid @ w1,
            "dw2": dpre2.t() @ act(hidden, 1), "db2": dpre2.sum(0), "dw1": dhid.t() @ pooled, "db1": dhid.sum(0)}


def stem_wgrad(du, z, kabc, x, N, H, W):
    """Weight gradient [32, 3, 3, 3] of the 3x3 stride-2 TF-SAME stem; x [N, H, W, 3], du / z [N*Ho*Wo, 32]."""
    (Ho, ph0, ph1), (Wo, pw0, pw1) = same_pad(H, 3, 2), same_pad(W, 3, 2)
    dz0 = nchw(kabc[0] * du + kabc[1] * z + kabc[2], N, Ho, Wo)
    xp = Fn.pad(x.permute(0, 3, 1, 2), (pw0, pw1, ph0, ph1))
    dw = torch.zeros(dz0.shape[1], 3, 3, 3, dtype=du.dtype)
    for kh in range(3):
        for kw in range(3):
            win = xp[:, :, kh:kh + (Ho - 1) * 2 + 1:2, kw:kw + (Wo - 1) * 2 + 1:2]
            dw[:, :, kh, kw] = torch.einsum("nohw,nihw->oi", dz0, win)
    return dw


def conv_weight_pack(w, ld):
    """torch [Co, Ci, k, k] -> [Co, ld], column (kh, kw, ci), zero padded (mt_conv_weight_pack, transpose = 0)."""
    Co = w.shape[0]
    out = torch.zeros(Co, ld, dtype=w.dtype)
    flat = w.permute(0, 2, 3, 1).reshape(Co, -1)
    out[:, :flat.shape[1]] = flat
    return out


def conv_weight_unpack(wp, Co, Ci, k):
    return wp[:, :k * k * Ci].reshape(Co, k, k, Ci).permute(0, 3, 1, 2).contiguous()
