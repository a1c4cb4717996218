"""The call layer (`lib.mt.<entry point>`) pins what it is handed: a tensor that reaches a recorded launch through it stays allocated
for as long as the plan lives -- also the device tables of the multi-tensor kernels, which used to go in as raw addresses."""
import pytest
import torch

from mintime_amd import lib as L
from mintime_amd import optim

pytestmark = pytest.mark.gpu


def test_recorded_call_pins_its_tensor():
    with L.Plan() as p:
        t = torch.full((1024,), 0xFF, dtype=torch.uint8, device="cuda")
        addr = t.data_ptr()
        L.mt.memset_async(t, 0, t.numel())
        del t
    assert p.ops == 1 and len(p.keep) == 1
    kept, = p.keep.values()
    assert kept.data_ptr() == addr and kept.dtype == torch.uint8 and kept.numel() == 1024
    torch.cuda.synchronize()
    assert int(kept.max()) == 0
    kept.fill_(0xFF)
    p.run()
    torch.cuda.synchronize()
    assert int(kept.max()) == 0


def test_recorded_sgd_step_pins_its_table():
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(8, device="cuda")) for _ in range(2)]
    p0 = [p.detach().clone() for p in ps]
    for p in ps:
        p.grad = torch.randn(8, device="cuda")
    opt = optim.FusedSGD(ps, lr=0.125)
    with L.Plan() as plan:
        opt.step()
    (table, _, _), = opt._tables.values()
    assert any(t is table for t in plan.keep.values())
    assert all(any(t is p for t in plan.keep.values()) for p in ps)
    plan.run()                                                   # the recorded step once more, through the kept table
    torch.cuda.synchronize()
    for p, q in zip(ps, p0):
        # two updates p -= lr * g, lr a power of two: two fp32 roundings (2^-24 relative each) of values below 8 in magnitude
        want = q.double() - 0.25 * p.grad.double()
        assert float(want.abs().max()) < 8.0
        torch.testing.assert_close(p.detach().double(), want, rtol=0, atol=2 * 8 * 2.0 ** -24)


def test_default_stream_is_the_current_stream_at_the_call():
    side = torch.cuda.Stream()
    assert L._current_stream() == torch.cuda.current_stream().cuda_stream
    with torch.cuda.stream(side):
        assert L._current_stream() == side.cuda_stream == L.stream_ptr().value
    assert L._current_stream() == torch.cuda.current_stream().cuda_stream != side.cuda_stream
