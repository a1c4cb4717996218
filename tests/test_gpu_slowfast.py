"""SlowFast R50 (`--model 2`) on the HIP path against the fp64 torch-CPU restatement of tests/slowfast_ref.py (the state-dict contract
of tests/golden/slowfast_r50_manifest.json, a hand-written manifest of pytorchvideo's structure).  Tolerances: twice the worst case
measured on an MI355X, rounded up (the measured values are next to each gate)."""
import pytest
import torch
import torch.nn.functional as F

import mintime_amd
from mintime_amd import lib as L, slowfast as S, slowfast_engine as E

from . import slowfast_ref as R
from .util import rel_err

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)

# (name, cin, cout, kernel, stride, padding) of every distinct convolution of the network
CONVS = [
    ("stem_slow", 3, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3)),
    ("stem_fast", 3, 8, (5, 7, 7), (1, 2, 2), (2, 3, 3)),
    ("fusion", 8, 16, (7, 1, 1), (4, 1, 1), (3, 0, 0)),
    ("conv_a_1", 80, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("conv_a_3", 32, 16, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ("conv_b", 16, 16, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("conv_b_s2", 16, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("conv_c", 16, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("branch1_s2", 32, 64, (1, 1, 1), (1, 2, 2), (0, 0, 0)),
]

CONV_TOL = 2e-6           # measured worst case over the sweep: 9.2e-7 (stem_fast forward)


def _rand_state(model, seed):
    g = torch.Generator().manual_seed(seed)
    sd = model.state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("running_var"):
            v.copy_(torch.rand(v.shape, generator=g) * 0.5 + 0.75)
        elif k.endswith("running_mean"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif "norm" in k and k.endswith(".weight"):
            v.copy_(torch.rand(v.shape, generator=g) * 0.6 + 0.7)
        elif "norm" in k and k.endswith(".bias"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif k.startswith("blocks.6.proj"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.05)
    return sd


def _model(seed=0, head=((8, 7, 7), (32, 7, 7)), classes=1):
    torch.manual_seed(seed)
    m = S.slowfast_r50(head_pool_kernel_sizes=head)
    m.blocks[6].proj = torch.nn.Linear(2304, classes)
    _rand_state(m, seed)
    ref = {k: v.detach().clone().double() for k, v in m.state_dict().items()}
    return m.to(dev), ref


def _videos(B, Fr, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, Fr, H, H, 3), generator=g, dtype=torch.uint8)


def _fm_from_ncdhw(x, cpad=None):
    """[N, C, T, H, W] CPU tensor -> Fm on the device (channels padded with zeros to cpad)."""
    N, Cc, T, H, W = x.shape
    t = x.permute(0, 2, 3, 4, 1).float()
    if cpad and cpad > Cc:
        t = F.pad(t, (0, cpad - Cc))
    return E.Fm(t.reshape(-1, t.shape[-1]).contiguous().to(dev), N, T, H, W)


def _to_ncdhw(fm, C=None):
    t = fm.t.detach().cpu().double().reshape(fm.N, fm.T, fm.H, fm.W, -1)
    if C is not None:
        t = t[..., :C]
    return t.permute(0, 4, 1, 2, 3)


# odd spatial sizes through the stride-2 convolutions: (name, cin, cout, kernel, stride, padding) at N = 1, (T, H, W) = (4, 7, 9)
ODD_CONVS = [
    ("conv_b_s2", 16, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("branch1_s2", 32, 64, (1, 1, 1), (1, 2, 2), (0, 0, 0)),
    ("stem_slow", 3, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3)),
]


@pytest.mark.parametrize("name,cin,cout,k,s,p", CONVS, ids=[c[0] for c in CONVS])
def test_conv3d_fwd_dgrad_wgrad(name, cin, cout, k, s, p):
    _conv_case(name, cin, cout, k, s, p, 2, (16 if name in ("stem_fast", "fusion") else 4), 18, 14)


@pytest.mark.parametrize("name,cin,cout,k,s,p", ODD_CONVS, ids=[c[0] for c in ODD_CONVS])
def test_conv3d_fwd_dgrad_wgrad_odd_sizes(name, cin, cout, k, s, p):
    _conv_case(name, cin, cout, k, s, p, 1, 4, 7, 9)


def _conv_case(name, cin, cout, k, s, p, N, T, H, W):
    torch.manual_seed(1)
    x = torch.randn(N, cin, T, H, W).double()                 # fp32 values: the device sees the same operands
    w = (torch.randn(cout, cin, *k) / (cin * k[0] * k[1] * k[2]) ** 0.5).double()
    stem = cin == 3
    pro = None
    xin = x
    if not stem:                                   # the BatchNorm + ReLU prologue on the loads
        sc = (torch.rand(cin) + 0.5).double()
        sh = (torch.randn(cin) * 0.3).double()
        pro = (sc.float().to(dev), sh.float().to(dev))
        xin = F.relu(x * sc[None, :, None, None, None] + sh[None, :, None, None, None])
    y_ref = F.conv3d(xin, w, stride=s, padding=p)
    xf = _fm_from_ncdhw(x, 4 if stem else None)
    conv = E.Conv("w", k, s, p)
    z, st = E.conv_fwd(xf, w.float().to(dev), conv, pro)
    torch.cuda.synchronize()
    e_fwd = rel_err(_to_ncdhw(z), y_ref)
    # BatchNorm sums of the output
    zr = _to_ncdhw(z)
    e_st = max(rel_err(st.cpu()[:cout], zr.sum((0, 2, 3, 4))), rel_err(st.cpu()[cout:], (zr * zr).sum((0, 2, 3, 4))))
    # weight gradient and data gradient against autograd of F.conv3d
    dy = torch.randn(y_ref.shape).double()
    xg = xin.detach().clone().requires_grad_(True)
    wg = w.detach().clone().requires_grad_(True)
    F.conv3d(xg, wg, stride=s, padding=p).backward(dy)
    dz = _fm_from_ncdhw(dy)
    dw = E.conv_wgrad(xf, pro, dz, w.float().to(dev), conv)
    e_w = rel_err(dw, wg.grad)
    e_d = 0.0
    if not stem:
        gx = torch.full((xf.rows, cin), float("nan"), device=dev)      # written, not accumulated: rows no tap reads get their zero too
        E.conv_dgrad(xf, dz, w.float().to(dev), conv, gx, False)
        e_d = rel_err(_to_ncdhw(E.Fm(gx, N, T, H, W)), xg.grad)
    torch.cuda.synchronize()
    print(f"conv {name} {(N, T, H, W)}: fwd {e_fwd:.2e} stats {e_st:.2e} wgrad {e_w:.2e} dgrad {e_d:.2e}")
    assert e_fwd <= CONV_TOL and e_st <= CONV_TOL and e_w <= CONV_TOL and e_d <= CONV_TOL, (e_fwd, e_st, e_w, e_d)


def test_conv3d_pitched_output_and_accumulate():
    """The fusion writes into a channel slice of a wider tensor; the data gradient accumulates into an existing gradient."""
    torch.manual_seed(2)
    x = torch.randn(1, 8, 16, 6, 6, dtype=torch.float64)
    w = torch.randn(16, 8, 7, 1, 1, dtype=torch.float64) * 0.1
    xf = _fm_from_ncdhw(x)
    cat = torch.full((1 * 4 * 6 * 6, 80), 7.0, device=dev)
    conv = E.Conv("w", (7, 1, 1), (4, 1, 1), (3, 0, 0))
    E.conv_fwd(xf, w.float().to(dev), conv, None, out=cat[:, 64:])
    ref = F.conv3d(x, w, stride=(4, 1, 1), padding=(3, 0, 0))
    got = cat[:, 64:].cpu().double().reshape(1, 4, 6, 6, 16).permute(0, 4, 1, 2, 3)
    assert rel_err(got, ref) <= CONV_TOL
    assert torch.all(cat[:, :64] == 7.0)
    g0 = torch.randn(xf.rows, 8, device=dev)
    g = g0.clone()
    dz = E.Fm(cat[:, 64:], 1, 4, 6, 6)
    E.conv_dgrad(xf, dz, w.float().to(dev), conv, g, True)
    xg = x.clone().requires_grad_(True)
    F.conv3d(xg, w, stride=(4, 1, 1), padding=(3, 0, 0)).backward(got)
    want = g0.cpu().double() + xg.grad.permute(0, 2, 3, 4, 1).reshape(-1, 8)
    assert rel_err(g, want) <= CONV_TOL


def test_ingest_matches_reference_transform():
    v = _videos(2, 16, 256, 3)
    slow, fast = mintime_amd.slowfast_input_transform(v)
    rs, rf = R.normalize_clip(v)
    assert slow.shape == rs.shape and fast.shape == rf.shape
    assert torch.equal(slow.cpu(), rs) and torch.equal(fast.cpu(), rf)
    # the [B, 3, F, H, W] layout of train.py:357 gives the same pair
    s2, f2 = mintime_amd.slowfast_input_transform(v.permute(0, 4, 1, 2, 3))
    assert torch.equal(s2.cpu(), rs) and torch.equal(f2.cpu(), rf)
    with pytest.raises(NotImplementedError):
        mintime_amd.slowfast_input_transform(_videos(1, 8, 128, 0))


EVAL_TOL = 2e-5           # measured: eval logits 6.9e-7, full-size train loss 8.8e-6


def test_eval_forward_full_size():
    m, ref = _model(seed=4, classes=3)
    m.eval()
    v = _videos(2, 16, 256, 5)
    rs, rf = R.normalize_clip(v)
    with torch.no_grad():
        y = m(mintime_amd.slowfast_input_transform(v))
        y2 = m([rs.to(dev), rf.to(dev)])                  # plain [B, 3, T, H, W] device tensors take the packing path
    yr = R.forward(ref, rs.double(), rf.double(), training=False)
    e = rel_err(y, yr)
    print(f"eval full size: logits rel err {e:.2e}")
    assert e <= EVAL_TOL
    assert torch.equal(y, y2)


SMALL_HEAD = ((4, 2, 2), (16, 2, 2))
# The reduced train step is badly conditioned where it is small (res5 normalises 48 values per channel at 64^2 and batch 3): torch's
# own fp32 CPU run of the restatement is ~0.2 off fp64 there.  Each tensor (logits, every parameter gradient, every running statistic)
# is therefore gated at T32_FACTOR times the torch-fp32 error of the same tensor, with a floor for the well-conditioned ones: the
# worst GPU error measured on an MI355X is 2.15x torch-fp32's (blocks.3...res_blocks.4.branch2.conv_c.weight), the gate twice that.
T32_FACTOR = 4.3
GRAD_FLOOR = 1e-4
GRAD_NORM_TOL = 5e-4      # full size, per-stage gradient norms: measured 2.4e-4 (blocks.0)


def _small_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    fast = torch.randn(B, 3, 16, 64, 64, generator=g)
    slow = fast[:, :, ::4].contiguous()
    return slow, fast


def _dropout(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g)


def _ref_step(ref, dt, slow, fast, labels, **kw):
    sd = {k: (v.to(dt) if v.is_floating_point() else v.clone()) for k, v in ref.items()}
    sd = {k: v.clone() for k, v in sd.items()}
    params = {k: v.requires_grad_(True) for k, v in sd.items() if not ("running" in k or "num_batches" in k)}
    y = R.forward(sd, slow.to(dt), fast.to(dt), training=True, **kw)
    loss = F.binary_cross_entropy_with_logits(y, labels.to(dt).reshape(-1, 1))
    loss.backward()
    return y, loss, {k: p.grad for k, p in params.items()}, sd


def test_train_step_small_all_gradients():
    m, ref = _model(seed=6, head=SMALL_HEAD)
    m.train()
    B = 3
    slow, fast = _small_inputs(B, 7)
    labels = torch.tensor([1.0, 0.0, 1.0])
    u = _dropout((B, 2304, 1, 1, 1), 8)
    m.dropout_uniform = lambda shape, device: u.to(device)
    y = m([slow.to(dev), fast.to(dev)])
    loss = F.binary_cross_entropy_with_logits(y, labels.to(dev).reshape(-1, 1))
    loss.backward()
    torch.cuda.synchronize()
    mult = (u.double() >= 0.5).double() / 0.5
    kw = dict(head_pool_kernel_sizes=SMALL_HEAD, dropout_mult=mult)
    yr, _, gr, sdr = _ref_step(ref, torch.float64, slow, fast, labels, **kw)
    y32, _, g32, sd32 = _ref_step(ref, torch.float32, slow, fast, labels, **{**kw, "dropout_mult": mult.float()})
    named = dict(m.named_parameters())
    buf = dict(m.named_buffers())
    checks = [("logits", y, y32, yr)] + [(k, named[k].grad, g32[k], gr[k]) for k in gr]
    checks += [(k, buf[k], sd32[k], sdr[k]) for k in sdr if "running" in k]
    worst, worst_k = 0.0, None
    for k, got, t32, want in checks:
        ratio = rel_err(got, want) / max(T32_FACTOR * rel_err(t32, want), GRAD_FLOOR)
        if ratio > worst:
            worst, worst_k = ratio, k
    e_y = rel_err(y, yr)
    print(f"train small: logits {e_y:.2e} (torch fp32 {rel_err(y32, yr):.2e}); worst error / gate {worst:.2f} ({worst_k})")
    assert worst <= 1.0, (worst, worst_k)
    assert {int(buf[k]) for k in buf if k.endswith("num_batches_tracked")} == {1}


def test_train_step_full_size_stage_gradients():
    m, ref = _model(seed=9)
    m.train()
    m.blocks[6].dropout.p = 0.0
    v = _videos(1, 16, 256, 10)
    labels = torch.tensor([1.0])
    y = m(mintime_amd.slowfast_input_transform(v))
    loss = F.binary_cross_entropy_with_logits(y, labels.to(dev).reshape(-1, 1))
    loss.backward()
    torch.cuda.synchronize()
    rs, rf = R.normalize_clip(v)
    _, lr, gr, _ = _ref_step(ref, torch.float64, rs, rf, labels)
    e_l = abs(loss.item() - lr.item()) / abs(lr.item())
    named = dict(m.named_parameters())
    errs = []
    for s in range(5):
        ks = [k for k in gr if k.startswith(f"blocks.{s}.")]
        gn = torch.sqrt(sum((named[k].grad.double().cpu() ** 2).sum() for k in ks))
        rn = torch.sqrt(sum((gr[k] ** 2).sum() for k in ks))
        errs.append(abs(gn - rn).item() / rn.item())
    print(f"train full size: loss rel err {e_l:.2e}, stage grad-norm rel errs {[f'{e:.2e}' for e in errs]}")
    assert e_l <= EVAL_TOL and max(errs) <= GRAD_NORM_TOL


def test_proj_swap_before_and_after_cuda():
    m = S.slowfast_r50(head_pool_kernel_sizes=SMALL_HEAD)
    m.blocks[6].proj = torch.nn.Linear(2304, 1)          # before .cuda() (train.py:146-147)
    m.to(dev).train()
    slow, fast = _small_inputs(2, 11)
    m.dropout_uniform = lambda shape, device: torch.ones(shape, device=device)
    y = m([slow.to(dev), fast.to(dev)])
    assert y.shape == (2, 1)
    y.sum().backward()
    assert m.blocks[6].proj.weight.grad is not None and m.blocks[6].proj.bias.grad is not None
    new = torch.nn.Linear(2304, 5).to(dev)                 # after .cuda(): the head reads whatever proj holds at call time
    m.blocks[6].proj = new
    m.zero_grad(set_to_none=True)
    y = m([slow.to(dev), fast.to(dev)])
    assert y.shape == (2, 5)
    y.sum().backward()
    assert new.weight.grad is not None and float(new.weight.grad.abs().sum()) > 0
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    w0 = new.weight.detach().clone()
    opt.step()
    assert not torch.equal(w0, new.weight.detach())


def test_frozen_backbone_and_eval_mode():
    m, _ = _model(seed=12, head=SMALL_HEAD)
    for n, p in m.named_parameters():
        if not n.startswith("blocks.6"):
            p.requires_grad_(False)
    m.train()
    slow, fast = _small_inputs(2, 13)
    m.dropout_uniform = lambda shape, device: torch.ones(shape, device=device)
    m([slow.to(dev), fast.to(dev)]).sum().backward()
    assert all(p.grad is None for n, p in m.named_parameters() if not n.startswith("blocks.6"))
    assert m.blocks[6].proj.weight.grad is not None


def _det_run():
    m, _ = _model(seed=14, head=SMALL_HEAD)
    m.train()
    slow, fast = _small_inputs(2, 15)
    m.dropout_uniform = lambda shape, device: _dropout(shape, 16).to(device)
    y = m([slow.to(dev), fast.to(dev)])
    y.sum().backward()
    return y.detach().cpu(), {n: p.grad.detach().cpu() for n, p in m.named_parameters()}


def test_deterministic_reruns_bit_identical():
    prev = L.set_deterministic(True)
    try:
        y0, g0 = _det_run()
        y1, g1 = _det_run()
    finally:
        L.set_deterministic(prev)
    assert torch.equal(y0, y1)
    assert all(torch.equal(g0[k], g1[k]) for k in g0)


def test_dataparallel_is_transparent():
    m, _ = _model(seed=17, head=SMALL_HEAD)
    m.eval()
    slow, fast = _small_inputs(2, 18)
    with torch.no_grad():
        y = m([slow.to(dev), fast.to(dev)])
        yd = torch.nn.DataParallel(m, device_ids=[0])([slow.to(dev), fast.to(dev)])
    assert torch.equal(y, yd)
    sd = torch.nn.DataParallel(m, device_ids=[0]).state_dict()
    assert all(k.startswith("module.") for k in sd)
    m2 = S.slowfast_r50(head_pool_kernel_sizes=SMALL_HEAD)
    m2.blocks[6].proj = torch.nn.Linear(2304, 1)
    m2.load_state_dict(sd)



def test_second_backward_and_replaced_or_updated_parameters_are_refused():
    """The saved walk was formed from the forward's parameters: a second backward, a parameter updated in place and a parameter whose
    storage was replaced after the forward are refused (plans.check_stamp)."""
    m, _ = _model(seed=2, head=SMALL_HEAD)
    m.train()
    slow, fast = _small_inputs(2, 3)
    x = [slow.to(dev), fast.to(dev)]
    y = m(x)
    y.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        y.sum().backward()
    w = m.blocks[6].proj.weight
    y = m(x)
    with torch.no_grad():
        w.mul_(2.0)
    with pytest.raises(RuntimeError, match="updated between"):
        y.sum().backward()
    y = m(x)
    w.data = w.data.clone()                          # same values, new storage: the version counter does not move
    with pytest.raises(RuntimeError, match="updated between"):
        y.sum().backward()
