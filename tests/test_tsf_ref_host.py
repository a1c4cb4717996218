"""tests/tsf_ref.py::attn_ref (the fp64 reference of tests/test_gpu_tsf_ops.py) against oracle/mintime_oracle.py::_attention, which
the reference fixtures of tests/test_oracle_golden.py validate: with identity projections the two are the same function."""
import pytest
import torch

from oracle import mintime_oracle as O

from . import tsf_ref as R


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H,Fr", [(1, 8), (2, 16)])
def test_attn_ref_equals_the_oracle_attention_under_identity_projections(H, Fr, mode):
    B, n, dh = 2, 49, 64
    inner, N = H * dh, 1 + Fr * n
    g = torch.Generator().manual_seed(10 * H + mode)
    qkv = torch.randn(B, N, 3 * inner, generator=g, dtype=torch.float64)
    mask = torch.rand(B, Fr, generator=g) < 0.7
    ident = torch.rand(B, Fr, Fr, generator=g) < 0.5
    assert not torch.equal(ident, ident.transpose(1, 2))
    sd = {"to_qkv.weight": torch.eye(3 * inner, dtype=torch.float64), "to_out.0.weight": torch.eye(inner, dtype=torch.float64),
          "to_out.0.bias": torch.zeros(inner, dtype=torch.float64)}
    fm = torch.nn.functional.pad(mask.unsqueeze(1).expand(B, Fr, Fr) & ident, (1, 0), value=True)
    frame_mask = fm.reshape(B, 1, 1, Fr, Fr + 1).expand(B, H, n, Fr, Fr + 1).reshape(B * H * n, Fr, Fr + 1)
    cm = torch.nn.functional.pad(mask.repeat_interleave(n, dim=1), (1, 0), value=True)
    cls_mask = cm.reshape(B, 1, 1, -1).expand(B, H, 1, N).reshape(B * H, 1, N)
    want, want_att = O._attention(qkv, sd, "", H, dh, "time" if mode == 0 else "space", n, Fr, frame_mask, cls_mask)
    got, got_att = R.attn_ref(qkv, mask, ident, H, Fr, n, mode, dh ** -0.5)
    assert float((got - want).abs().max()) <= 1e-12
    assert float((got_att - want_att.reshape(B * H, N)).abs().max()) <= 1e-12
    # mode 2 is the cls query of either mode, alone
    cls_only, att2 = R.attn_ref(qkv, mask, ident, H, Fr, n, 2, dh ** -0.5)
    assert torch.equal(cls_only[:, 0], got[:, 0]) and torch.equal(att2, got_att) and float(cls_only[:, 1:].abs().max()) == 0.0
