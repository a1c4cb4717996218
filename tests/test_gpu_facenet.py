"""The FaceNet InceptionResnetV1 embedder on the device (mintime_amd.facenet) against the fp64 restatement tests/facenet_ref.py.

The gate is not a fixed number: on the same weights and crops the test computes e32 = max |fp32 CPU restatement - fp64| and requires
max |HIP - fp64| <= 4 * e32.  The margin is there because a k-ordered fmaf chain over up to 2304 terms grows differently from
oneDNN's blocked sums; the ratio is expected near 1-2 (measured ratios: profiles/facenet_parity.txt).  A case is valid only when
the fp64 embeddings of its distinct crops have cosine below 0.999 -- otherwise the weights are degenerate and it proves nothing."""
import numpy as np
import pytest
import torch

import mintime_amd
from mintime_amd import facenet_engine as E
from tests import facenet_ref as R
from tests import identity_ref as IR

pytestmark = pytest.mark.gpu

SEED = 0
_CACHE = {}


def state(seed=SEED):
    if ("sd", seed) not in _CACHE:
        _CACHE[("sd", seed)] = R.seeded_state(seed)
    return _CACHE[("sd", seed)]


def model(seed=SEED):
    if ("model", seed) not in _CACHE:
        m = mintime_amd.InceptionResnetV1()
        m.load_state_dict(state(seed))
        _CACHE[("model", seed)] = m.cuda().eval()
    return _CACHE[("model", seed)]


def crops(T, H, W, seed):
    return torch.randint(0, 256, (T, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def reference(c, seed=SEED):
    """(fp64 embeddings, e32) of uint8 crops [T, H, W, 3] under the seeded weights, computed once per input."""
    key = ("ref", seed, tuple(c.shape), int(c.long().sum()))
    if key not in _CACHE:
        x = R.standardize(c.permute(0, 3, 1, 2).double())
        e64 = R.forward(R.to_dtype(state(seed), torch.float64), x)
        e32 = R.forward(state(seed), x.float())
        _CACHE[key] = (e64, (e32.double() - e64).abs().max().item())
    return _CACHE[key]


@pytest.mark.parametrize("T,H,W", [(3, 80, 80), (2, 128, 128), (1, 75, 76)])
def test_embeddings_against_fp64(T, H, W):
    c = crops(max(T, 2), H, W, 100 + H)              # (a second crop for the validity condition of the T = 1 case)
    e64, e32 = reference(c)
    cos = (e64 @ e64.T).fill_diagonal_(0).abs().max().item()
    assert cos < 0.999, f"degenerate weights: distinct crops at cosine {cos}"
    c = c[:T]
    got = model().embed_crops(c.cuda()).cpu().double()
    assert got.shape == (T, 512) and got.dtype == torch.float64
    err = (got - e64[:T]).abs().max().item()
    print(f"facenet parity {T} x {H} x {W}: HIP err {err:.3e}, fp32 CPU err (e32) {e32:.3e}, ratio {err / e32:.2f}")
    assert (got.norm(dim=1) - 1).abs().max().item() < 1e-6
    assert err <= 4 * e32, (err, e32)


def test_output_has_no_grad_fn_and_small_faces_raise():
    m = model()
    x = R.standardize(crops(1, 80, 80, 1).permute(0, 3, 1, 2).float()).cuda().requires_grad_(True)
    y = m(x)
    assert y.grad_fn is None and not y.requires_grad and y.is_cuda and y.dtype == torch.float32
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 74, 80, device="cuda"))
    with pytest.raises(ValueError):
        m.embed_crops(torch.zeros(1, 80, 74, 3, dtype=torch.uint8, device="cuda"))
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m(x)
    finally:
        m.eval()


def test_embed_crops_equals_forward_of_the_standardised_tensor():
    m = model()
    c = crops(3, 80, 77, 2).cuda()
    a = m.embed_crops(c).clone()
    nhwc = mintime_amd.fixed_image_standardization(c.float())
    view = nhwc.permute(0, 3, 1, 2)                                   # predict.py:154: the zero-copy channels-last view
    assert not view.is_contiguous()
    b = m(view).clone()
    assert torch.equal(a, b)
    assert torch.equal(m(view.contiguous()).clone(), b)              # NCHW-contiguous input: the same bits
    assert torch.equal(m.embed_crops(c.float()).clone(), a)          # raw fp32 crops


def test_a_face_does_not_depend_on_its_batch():
    m = model()
    c = crops(5, 80, 80, 3).cuda()
    five = m.embed_crops(c).clone()
    for i in (0, 3):
        assert torch.equal(m.embed_crops(c[i:i + 1]).clone(), five[i:i + 1])


def test_a_batch_of_chunk_plus_one_equals_its_chunks():
    m = model()
    n = m.engine().chunk
    assert n == E.CHUNK
    c = crops(n + 1, 75, 75, 4).cuda()
    whole = m.embed_crops(c).clone()
    assert torch.equal(whole[:n], m.embed_crops(c[:n]).clone())
    assert torch.equal(whole[n:], m.embed_crops(c[n:]).clone())
    assert torch.isfinite(whole).all()


def test_no_allocation_after_the_first_call_at_a_shape():
    m = model()
    c = crops(2, 80, 80, 5).cuda()
    first = m.embed_crops(c)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    again = m.embed_crops(c)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert again.data_ptr() == first.data_ptr()


def test_load_state_dict_refolds_the_weights():
    m = mintime_amd.InceptionResnetV1()
    m.load_state_dict(state(0))
    m = m.cuda().eval()
    c = crops(2, 80, 80, 6).cuda()
    old = m.embed_crops(c).clone()
    assert torch.equal(old, model(0).embed_crops(c))
    m.load_state_dict(state(1))
    new = m.embed_crops(c).clone()
    assert not torch.equal(new, old)
    assert torch.equal(new, model(1).embed_crops(c))
    with torch.no_grad():
        m.last_bn.bias.add_(0.25)                                     # an in-place edit refolds too
    assert not torch.equal(m.embed_crops(c), new)


def test_into_the_clustering():
    g = torch.Generator().manual_seed(7)
    base = torch.randint(0, 256, (3, 80, 80, 3), generator=g)
    order = [0, 1, 0, 2, 1, 0, 2, 1, 2]
    c = torch.stack([(base[i] + torch.randint(-3, 4, (80, 80, 3), generator=g)).clamp(0, 255) for i in order]).to(torch.uint8)
    e64, e32 = reference(c)
    sim = (e64 @ e64.T).numpy()
    off = np.sort(sim[np.triu_indices(len(order), 1)])
    i = int(np.argmax(np.diff(off)))
    gap, thr = off[i + 1] - off[i], 0.5 * (off[i] + off[i + 1])
    assert gap > 100 * 4 * e32, f"input rejected: the largest gap {gap} is within 100 gates ({4 * e32}) "
    want, n_ids, _ = IR.cluster_embeddings(e64.numpy(), [len(order)], thr)
    assert n_ids[0] == 3 and list(want) == order                      # three identities, numbered by first appearance
    plan = mintime_amd.ClusterPlan([len(order)], 512)
    got = plan.run(model().embed_crops(c.cuda()), float(thr))
    assert list(got.host_labels()) == list(want)
