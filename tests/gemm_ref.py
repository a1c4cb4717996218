"""The semantics of mt_gemm's descriptor (include/mintime_hip.h, "Dense contraction family") in plain torch on the CPU, written from
the header and not from the kernels.  gemm() takes the arguments of mintime_amd.lib.gemm -- CPU tensors where that takes device
tensors, each a view that STARTS at the operand's base element; shapes and leading dimensions come from the arguments, as in the
ABI -- and returns every output the call writes.  The arithmetic runs in the dtype of A: float64 for the reference, float32 for the
yardstick of the GPU tests (tests/test_gpu_gemm_ops.py); with a gathered A operand (PRO_IM2COL), whose image may be uint8, in the
dtype of B.  tests/test_gemm_ref_host.py ties the fused forms to torch autograd and the im2col forms to F.conv2d."""
import math

import torch

OP_NT, OP_NN, OP_TN = 0, 1, 2
PRO_NONE, PRO_BN_SWISH_GATE, PRO_BN_BWD, PRO_IM2COL = 0, 1, 4, 5
BPRO_NONE, BPRO_BN_SWISH_GATE, BPRO_IM2COL = 0, 1, 2
ACT_NONE, ACT_RELU = 0, 2                     # conv_act
(EPI_STORE, EPI_BIAS_RES, EPI_GEGLU, EPI_STATS, EPI_ATOMIC, EPI_GEGLU_BWD, EPI_ACCUM, EPI_SE_RED, EPI_ACT_BWD) = range(9)


def map_rows(rmap, rows):
    """mt_rowmap: row' = (r / gin) * gout + off + r % gin; gin == 0: identity."""
    r = torch.arange(rows)
    gin, gout, off = rmap
    return r if gin == 0 else (r // gin) * gout + off + r % gin


def mat(t, rows, cols, ld, rmap=(0, 0, 0)):
    """[rows, cols] view of the operand whose base element is t's first: element (r, c) = base[map(r) * ld + c]."""
    idx = map_rows(rmap, rows)
    v = torch.as_strided(t, (int(idx.max()) + 1, cols), (ld, 1), t.storage_offset())
    return v if rmap[0] == 0 else v[idx]


def swish(u):
    return u * torch.sigmoid(u)


def dswish(u):
    s = torch.sigmoid(u)
    return s * (1 + u * (1 - s))


def gelu(g):
    return 0.5 * g * (1 + torch.erf(g / math.sqrt(2.0)))


def dgelu(g):
    return 0.5 * (1 + torch.erf(g / math.sqrt(2.0))) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def im2col(x, conv, rows, cols, scale, shift, dt):
    """The virtual matrix of MT_PRO_IM2COL / MT_BPRO_IM2COL, [rows, cols] in dtype dt, from the dense NHWC image (fp32 or uint8) whose
    first element is x's first; conv = (H, W, C, Ho, Wo, k, stride, pad, act[, src_u8]):
      row (n, oh, ow), column (kh, kw, ci) = act(x[n, oh s + kh - p, ow s + kw - p, ci] scale[ci] + shift[ci])
    and exactly zero where the tap lies outside the image (the padding passes through neither the affine nor the activation) and in
    the columns from k k C on.  Ho and Wo are taken as given: a window may hang over the bottom / right edge."""
    H, W, C, Ho, Wo, k, s, p, act = conv[:9]
    n_img = (rows - 1) // (Ho * Wo) + 1
    img = x.reshape(-1)[:n_img * H * W * C].to(dt).reshape(n_img, H, W, C)
    r = torch.arange(rows)
    n, oh, ow = r // (Ho * Wo), (r // Wo) % Ho, r % Wo
    out = torch.zeros(rows, cols, dtype=dt)
    for kh in range(k):
        for kw in range(k):
            ih, iw = oh * s + kh - p, ow * s + kw - p
            ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
            v = img[n[ok], ih[ok], iw[ok]]
            if scale is not None:
                v = v * scale.to(dt)[:C] + shift.to(dt)[:C]
            if act == ACT_RELU:
                v = v.clamp_min(0)
            elif act != ACT_NONE:
                raise ValueError(f"conv_act {act} is not covered")
            c0 = (kh * k + kw) * C
            out[ok, c0:c0 + C] = v
    return out


def operands(op, A, B, M, N, K, lda, ldb, prologue=PRO_NONE, scale=None, shift=None, gate=None, hw=1, a_map=(0, 0, 0),
             b_map=(0, 0, 0), A2=None, b_prologue=BPRO_NONE, b_scale=None, b_shift=None, b_gate=None, b_hw=1, conv=None, **_):
    """The two factors after their prologues, a [M, K] and b [K, N], in A's dtype (B's when A is a gathered image)."""
    dt = B.dtype if prologue == PRO_IM2COL else A.dtype

    def load_a(t):
        return mat(t, K, M, lda, a_map).T if op == OP_TN else mat(t, M, K, lda, a_map)

    if prologue == PRO_IM2COL:                  # NT only: rows = output pixels, K = k k C padded to a multiple of 4
        assert op == OP_NT
        a = im2col(A, conv, M, K, scale, shift, dt)
    else:
        a = load_a(A)
    if b_prologue == BPRO_IM2COL:               # TN only: the contraction runs over the output pixels, columns = padded k k C
        assert op == OP_TN
        b = im2col(B, conv, K, N, b_scale, b_shift, dt)
    else:
        b = mat(B, N, K, ldb).T if op == OP_NT else mat(B, K, N, ldb, b_map)    # b_map: rows of a k-major B only
    if prologue == PRO_BN_SWISH_GATE:           # a = swish(z scale[k] + shift[k]) gate[m / hw, k]
        g = mat(gate, (M - 1) // hw + 1, K, K).to(dt)
        a = swish(a * scale.to(dt) + shift.to(dt)) * g.repeat_interleave(hw, 0)[:M]
    elif prologue == PRO_BN_BWD:                # a = ka[c] A + kb[c] A2 + kc[c]; c = the channel: k, or the output row m of TN
        ka, kb, kc = (v.to(dt)[:M, None] if op == OP_TN else v.to(dt)[:K] for v in (scale, shift, gate))
        a = ka * a + kb * load_a(A2) + kc
    elif prologue not in (PRO_NONE, PRO_IM2COL):
        raise ValueError(f"prologue {prologue} is not covered")
    if b_prologue == BPRO_BN_SWISH_GATE:        # TN only: b = swish(B b_scale[n] + b_shift[n]) b_gate[k / b_hw, n]
        assert op == OP_TN
        g = mat(b_gate, (K - 1) // b_hw + 1, N, N).to(dt)
        b = swish(b * b_scale.to(dt)[:N] + b_shift.to(dt)[:N]) * g.repeat_interleave(b_hw, 0)[:K]
    elif b_prologue not in (BPRO_NONE, BPRO_IM2COL):
        raise ValueError(f"B prologue {b_prologue} is not covered")
    return a, b


def gemm(op, A, B, Cout, M, N, K, lda, ldb, ldc, prologue=PRO_NONE, epilogue=EPI_STORE, bias=None, R=None, ldr=0, scale=None,
         shift=None, gate=None, hw=1, C2=None, ldc2=0, stats=None, stats_slots=1, n_half=0, split_k=1, a_map=(0, 0, 0),
         b_map=(0, 0, 0), c_map=(0, 0, 0), A2=None, b_prologue=BPRO_NONE, b_scale=None, b_shift=None, b_gate=None, b_hw=1,
         col_sum=None, epi=None, conv=None):
    """{name: tensor} of what the call leaves behind:
      C        the output rows in LOGICAL order (row m = memory row c_map(m)); [M, N], GEGLU [M, n_half], GEGLU_BWD [M, 2 n_half],
               SE_RED [M / e_hw, N]; accumulating epilogues (BIAS_RES in place, ATOMIC, ACCUM, SE_RED) start from what Cout holds
      C2       GEGLU: the interleaved pre-activations [M, 2 n_half]
      stats    STATS / ACT_BWD: the two column sums [2, N] that the call ADDS to the accumulators (over all slots)
      col_sum  GEGLU_BWD: col_sum's new value [2 n_half]
    and, for every summed output, `<name>_abs`: the sum of the terms' magnitudes (the conditioning of the sum)."""
    a, b = operands(op, A, B, M, N, K, lda, ldb, prologue, scale, shift, gate, hw, a_map, b_map, A2, b_prologue, b_scale, b_shift,
                    b_gate, b_hw, conv)
    dt = a.dtype
    if prologue == PRO_IM2COL and epilogue not in (EPI_STORE, EPI_STATS):
        raise ValueError(f"im2col A with epilogue {epilogue} is not covered")
    if b_prologue == BPRO_IM2COL and (prologue, epilogue) != (PRO_BN_BWD, EPI_ATOMIC):
        raise ValueError(f"im2col B with prologue {prologue} / epilogue {epilogue} is not covered")
    acc = a @ b
    bv = bias.to(dt)[:N] if bias is not None else torch.zeros(N, dtype=dt)
    out = {}
    if epilogue == EPI_STORE:
        out["C"] = acc + bv
    elif epilogue == EPI_BIAS_RES:
        out["C"] = acc + bv + mat(R, M, N, ldr, c_map).to(dt)
    elif epilogue in (EPI_ATOMIC, EPI_ACCUM):
        out["C"] = mat(Cout, M, N, ldc, c_map).to(dt) + acc + bv
    elif epilogue == EPI_STATS:
        out["C"] = acc
        out["stats"] = torch.stack((acc.sum(0), (acc * acc).sum(0)))
        out["stats_abs"] = torch.stack((acc.abs().sum(0), (acc * acc).sum(0)))
    elif epilogue == EPI_GEGLU:
        assert N == 2 * n_half
        u = acc + bv
        av, gv = u[:, :n_half], u[:, n_half:]
        out["C"] = av * gelu(gv)
        out["C2"] = torch.stack((av, gv), dim=-1).reshape(M, N)
    elif epilogue == EPI_GEGLU_BWD:
        assert N == n_half
        u = mat(C2, M, 2 * n_half, ldc2).to(dt).reshape(M, n_half, 2)
        av, gv = u[..., 0], u[..., 1]
        du = torch.cat((acc * gelu(gv), acc * av * dgelu(gv)), dim=1)
        out["C"] = du
        if col_sum is not None:
            out["col_sum"] = col_sum.to(dt)[:2 * n_half] + du.sum(0)
            out["col_sum_abs"] = du.abs().sum(0)
    elif epilogue in (EPI_SE_RED, EPI_ACT_BWD):
        e_scale, e_shift, e_gate, e_dpool, e_mi, e_hw = epi
        n_img = (M - 1) // e_hw + 1
        img = torch.arange(M) // e_hw
        z = mat(C2, M, N, ldc2).to(dt)
        u = z * e_scale.to(dt)[:N] + e_shift.to(dt)[:N]
        if epilogue == EPI_SE_RED:
            t = acc * swish(u)
            c0 = mat(Cout, n_img, N, ldc).to(dt)
            out["C"] = c0.index_add(0, img, t)
            out["C_abs"] = torch.zeros_like(c0).index_add(0, img, t.abs())
        else:
            g, dp = mat(e_gate, n_img, N, N).to(dt)[img], mat(e_dpool, n_img, N, N).to(dt)[img]
            du = (acc * g + dp / e_hw) * dswish(u)
            mi = e_mi.to(dt)
            t2 = du * (z - mi[:N]) * mi[N:2 * N]
            out["C"] = du
            out["stats"] = torch.stack((du.sum(0), t2.sum(0)))
            out["stats_abs"] = torch.stack((du.abs().sum(0), t2.abs().sum(0)))
    else:
        raise ValueError(f"epilogue {epilogue} is not covered")
    return out
