"""Host side of the identity clustering: the restatement the GPU tests compare against (tests/identity_ref.py) is held to the
outputs of the reference's _generate_connected_components recorded in tests/golden/identity_components.json; the three entry points
are declared and bound; the host grouping feeds sequence.plan_clip; argument errors raise before the library is touched.  No device
is touched."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import mintime_amd
from mintime_amd import identities as I
from mintime_amd import lib as L
from mintime_amd import sequence as S
from tests import identity_ref as R
from tests.util import GOLDEN, declared_params, header_text


def fixture_cases():
    with open(os.path.join(GOLDEN, "identity_components.json")) as fh:
        rows = json.load(fh)
    for r in rows:
        sim = np.array([[np.nan if x is None else x for x in row] for row in r["similarities"]], dtype=np.float32)
        r["similarities"] = sim.reshape(r["n"], r["n"])
    return rows


CASES = fixture_cases()


def test_fixture_covers_the_cases_the_rule_turns_on():
    names = {c["name"] for c in CASES}
    assert len(CASES) >= 20 and all(c["n"] <= 40 for c in CASES)
    assert {"one_face", "asymmetric", "random_asymmetric", "at_threshold", "nan_entries", "zero_matrix_negative_threshold"} <= names
    by = {c["name"]: c for c in CASES}
    assert by["one_face"]["n"] == 1 and by["one_face"]["components"] == []
    assert np.isnan(by["nan_entries"]["similarities"]).any()
    s = by["at_threshold"]["similarities"]
    assert (s == np.float32(by["at_threshold"]["threshold"])).any()
    a = by["asymmetric"]["similarities"]
    assert not np.array_equal(a, a.T)
    assert by["zero_matrix_negative_threshold"]["threshold"] < 0 and not by["zero_matrix_negative_threshold"]["similarities"].any()
    assert any(len(c["components"]) >= 3 for c in CASES)
    assert any(sum(len(m) for m in c["components"]) < c["n"] and c["components"] for c in CASES)      # edgeless faces next to identities


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_the_recorded_reference_output(case):
    labels, n_ids, sizes = R.cluster_similarities(case["similarities"], case["threshold"])
    want = case["components"]
    assert R.components_from_labels(labels) == want                     # order included
    assert n_ids == len(want)
    assert sizes.tolist() == [len(c) for c in want] + [0] * (case["n"] - len(want))
    in_some = {i for c in want for i in c}
    assert [i for i in range(case["n"]) if labels[i] < 0] == [i for i in range(case["n"]) if i not in in_some]


def test_component_order_on_an_asymmetric_matrix_follows_the_first_source_row():
    """Entry (2, 0) alone joins {0, 2}; entry (1, 3) alone joins {1, 3}.  The reference's loop adds the edge 1 -- 3 at row 1 and the
    edge 2 -- 0 at row 2, so networkx lists [1, 3] first although 0 is the smallest member overall.  Symmetrised, the order is by
    smallest member."""
    s = np.zeros((4, 4), np.float32)
    s[2, 0] = s[1, 3] = 1.0
    labels, n_ids, sizes = R.cluster_similarities(s, 0.5)
    assert labels.tolist() == [1, 0, 1, 0] and n_ids == 2 and sizes.tolist() == [2, 2, 0, 0]
    labels, _, _ = R.cluster_similarities(np.maximum(s, s.T), 0.5)
    assert labels.tolist() == [0, 1, 0, 1]


def test_gram_restatement_hand_case():
    """D = 1, e = [1, 1, -1, 0.5], threshold 0.45: s_01 = 1, s_03 = s_13 = 0.5 join {0, 1, 3}; face 2 only has negative products."""
    e = np.array([[1.0], [1.0], [-1.0], [0.5]])
    labels, n_ids, sizes = R.cluster_embeddings(e, [4], 0.45)
    assert labels.tolist() == [0, 0, -1, 0] and n_ids.tolist() == [1] and sizes.tolist() == [3, 0, 0, 0]
    assert R.min_margin(e, [4], 0.45) == pytest.approx(0.05, abs=1e-6)
    # ragged: the same rows as two videos never join across the boundary
    labels, n_ids, _ = R.cluster_embeddings(e, [1, 3], 0.45)
    assert labels.tolist() == [-1, 0, -1, 0] and n_ids.tolist() == [0, 1]


def test_unpack_adjacency():
    w = np.array([[1, 0], [-2147483648, 3]], dtype=np.int32)
    b = R.unpack_adjacency(w)
    assert b.shape == (2, 64)
    assert np.nonzero(b[0])[0].tolist() == [0] and np.nonzero(b[1])[0].tolist() == [31, 32, 33]


@pytest.mark.parametrize("name,count", [("mt_identity_adjacency", 12), ("mt_identity_adjacency_sim", 6), ("mt_identity_components", 11)])
def test_entry_point_is_declared_and_bound(name, count):
    params = declared_params(name)
    assert params[-1] == "void* stream"                          # a launching entry point: csrc/gen_plan.py gives it a recording thunk
    assert name in L.PROTOTYPES and len(L.PROTOTYPES[name]) == len(params) == count
    handle = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(handle, name) and hasattr(handle, "mti_" + name[3:])


def test_package_surface_limits_and_abi_number():
    for name in ("ClusterPlan", "IdentityClusters", "cluster_embeddings", "cluster_similarities", "identities_from_labels"):
        assert getattr(mintime_amd, name) is getattr(mintime_amd.identities, name) and name in mintime_amd.__all__
    assert (I.MAX_FACES, I.MAX_DIM, I.TILE) == (4096, 2048, 32)
    hdr = header_text()
    decl = hdr[hdr.index("Identity clustering"):hdr.index("int mt_identity_components")]
    for cited in ("preprocessing/utils.py:16-29", "cluster_faces.py", "predict.py", "4096", "2048"):
        assert cited in decl
    assert L.ABI_VERSION == 123
    assert re.search(r"#define\s+MT_VERSION\s+(\d+)", hdr).group(1) == "123"


FACES = [(30, 50, 40), (10, 52, 44), (20, 20, 16), (40, 48, 36), (50, 22, 18), (60, 90, 80)]


def test_identities_from_labels_on_a_toy_batch():
    """Video 0 is empty; video 1 has six faces: identity 0 = {1, 3, 0}, identity 1 = {2, 4}, face 5 without an identity."""
    labels = [0, 0, 1, 0, 1, -1]
    (ids0, disc0), (ids1, disc1) = I.identities_from_labels(labels, [0, 0, 6], [[], FACES])
    assert ids0 == [] and disc0 == []
    assert [i.name for i in ids1] == ["0", "1"] and disc1 == [5]
    assert ids1[0].faces == [FACES[0], FACES[1], FACES[3]] and ids1[1].faces == [FACES[2], FACES[4]]       # index order
    assert all(isinstance(i, S.Identity) for i in ids1)
    with pytest.raises(ValueError):
        I.identities_from_labels(labels, [0, 0, 6], [[], FACES[:5]])
    with pytest.raises(ValueError):
        I.identities_from_labels(labels, [0, 0, 6], [FACES])


def test_grouping_goes_into_plan_clip_unchanged():
    (_, _), (ids, _) = I.identities_from_labels([0, 0, 1, 0, 1, -1], [0, 0, 6], [[], FACES])
    plan = S.plan_clip(ids, num_frames=8, video_wh=(640, 480), max_identities=2, ordering=1)
    # two identities of 3 and 2 faces in 8 frames: caps 4 + 4; the first hands its unused slot on, the last is padded to the end
    assert [i.name for i in plan.identities] == ["0", "1"] and [i.slots for i in plan.identities] == [3, 5]
    assert plan.chosen[0] == sorted(ids[0].faces) and plan.chosen[1] == sorted(ids[1].faces)              # temporal order
    by_side = S.plan_clip(ids, num_frames=8, video_wh=(640, 480), max_identities=1, ordering=0)
    assert [i.name for i in by_side.identities] == ["0"] and by_side.identities[0].slots == 8              # mean width 40 against 17


def test_argument_errors_raise_before_the_library_is_touched(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "get", touched)
    e = torch.zeros(6, 8)
    with pytest.raises(ValueError, match="no CPU path"):
        I.ClusterPlan([6], 8, device="cpu")
    with pytest.raises(ValueError, match="no CPU path"):
        I.cluster_embeddings(e, [6])
    with pytest.raises(ValueError, match="no CPU path"):
        I.cluster_similarities(torch.zeros(4, 4))
    with pytest.raises(ValueError, match="no CPU path"):
        I.cluster_embeddings(e.numpy(), [6])
    with pytest.raises(NotImplementedError, match="4096"):
        I.cluster_embeddings(e, [4097])
    with pytest.raises(NotImplementedError, match="4096"):
        I.ClusterPlan([1, 4097], 8)
    with pytest.raises(NotImplementedError, match="2048"):
        I.ClusterPlan([6], 2049)
    with pytest.raises(NotImplementedError, match="2048"):
        I.ClusterPlan([6], 0)
    with pytest.raises(ValueError):
        I.ClusterPlan([], 8)
    with pytest.raises(ValueError):
        I.ClusterPlan([3, -1], 8)
    # the tensor checks themselves, on a host tensor that claims to be on the device
    with pytest.raises(ValueError, match="fp32"):
        I._check_embeddings(_FakeDeviceTensor(torch.zeros(6, 8, dtype=torch.float64)), [6])
    with pytest.raises(ValueError, match="add up to 5"):
        I._check_embeddings(_FakeDeviceTensor(e), [2, 3])
    with pytest.raises(ValueError, match="dim = 16"):
        I._check_embeddings(_FakeDeviceTensor(e), [6], 16)
    I._check_embeddings(_FakeDeviceTensor(e), [2, 4], 8)


class _FakeDeviceTensor(torch.Tensor):
    """A host tensor that answers is_cuda with True: reaches the dtype / shape checks without a device."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def test_error_flag_text():
    with pytest.raises(L.MintimeHipError, match="truncated"):
        I._raise_on_flag(I.ERR_TRUNCATED)
    with pytest.raises(L.MintimeHipError, match="trip bound"):
        I._raise_on_flag(I.ERR_NOT_CONVERGED | I.ERR_TRUNCATED)
    I._raise_on_flag(0)
