"""Plain-torch restatement of the divided-attention core (csrc/tsf_fwd.hip mt_attn_fwd and its adjoint), written from the operation's
definition on the kernels' own layout: qkv [B, N, 3*H*64] in, merged heads [B, N, H*64] out.  It follows
oracle/mintime_oracle.py::_attention without the two Linear layers (tests/test_tsf_ref_host.py ties the two together); any dtype,
fp64 in the tests.  The backward is torch autograd of it."""
import torch

DH = 64
NEG = -torch.finfo(torch.float32).max            # the fill value of masked logits (fill, not add)


def _softmax_av(q, k, v, keep):
    """q [..., I, d], k / v [..., J, d], keep [..., I, J] bool or None -> (out [..., I, d], p [..., I, J])."""
    s = q @ k.transpose(-1, -2)
    if keep is not None:
        s = s.masked_fill(~keep, NEG)
    p = s.softmax(-1)
    return p @ v, p


def attn_ref(qkv, mask, ident, H, F, n, mode, scale):
    """qkv [B, N, 3*H*64], mask [B, F] bool, ident [B, F, F] bool; mode 0 = time, 1 = space, 2 = the cls query alone.
    Returns (out [B, N, H*64], cls_att [B*H, N]); in mode 2 the patch rows of out are zeros (the kernel does not write them)."""
    B, N, _ = qkv.shape
    assert N == 1 + F * n
    q, k, v = (t.reshape(B, N, H, DH).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))     # [B, H, N, d]
    q = q * scale
    # the cls query: every key, padded frames masked, the cls key always kept
    cls_keep = torch.cat((torch.ones(B, 1, dtype=torch.bool), mask.bool().repeat_interleave(n, dim=1)), dim=1)     # [B, N]
    cls_out, cls_p = _softmax_av(q[:, :, :1], k, v, cls_keep[:, None, None, :])                # [B, H, 1, d], [B, H, 1, N]
    cls_att = cls_p.reshape(B * H, N)
    if mode == 2:
        out = torch.cat((cls_out, torch.zeros_like(q[:, :, 1:])), dim=2)
        return out.permute(0, 2, 1, 3).reshape(B, N, H * DH), cls_att
    qp, kp, vp = (t[:, :, 1:].reshape(B, H, F, n, DH) for t in (q, k, v))
    ck = k[:, :, :1].unsqueeze(2)                                                              # [B, H, 1, 1, d]
    cv = v[:, :, :1].unsqueeze(2)
    if mode == 0:            # groups (b, h, patch): F queries, keys = cls + the same patch over the F frames
        qg, kg, vg = (t.transpose(2, 3) for t in (qp, kp, vp))                                 # [B, H, n, F, d]
        keep = mask.bool()[:, None, :] & ident.bool()                                          # [B, F(query), F(key)]
        keep = torch.cat((torch.ones(B, F, 1, dtype=torch.bool), keep), dim=2)[:, None, None]  # [B, 1, 1, F, F + 1]
        G = n
    else:                    # groups (b, h, frame): n queries, keys = cls + the same frame's n patches, no mask
        qg, kg, vg, keep, G = qp, kp, vp, None, F
    kg = torch.cat((ck.expand(B, H, G, 1, DH), kg), dim=3)
    vg = torch.cat((cv.expand(B, H, G, 1, DH), vg), dim=3)
    og, _ = _softmax_av(qg, kg, vg, keep)
    if mode == 0:
        og = og.transpose(2, 3)                                                                # back to [B, H, F, n, d]
    out = torch.cat((cls_out, og.reshape(B, H, F * n, DH)), dim=2)
    return out.permute(0, 2, 1, 3).reshape(B, N, H * DH), cls_att


def attn_bwd_ref(qkv, dout, mask, ident, H, F, n, mode, scale):
    """d(out * dout).sum() / d qkv by autograd (mode 2: the loss reads row 0 of every clip only)."""
    x = qkv.detach().clone().requires_grad_(True)
    out, _ = attn_ref(x, mask, ident, H, F, n, mode, scale)
    if mode == 2:
        (out[:, 0] * dout[:, 0]).sum().backward()
    else:
        (out * dout).sum().backward()
    return x.grad
