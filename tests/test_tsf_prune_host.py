"""Host-side checks of the last-layer dead-row pruning on the plane path: the two entry points are declared, bound and get recording
thunks; the switch's default and its exceptions (tsf_planes.prune_last / eligible)."""
import types

import pytest

from mintime_amd import lib as L
from mintime_amd import tsf_planes

from .util import declared_params, header_text


@pytest.mark.parametrize("name,nparams", [("mt_attn_bwd_cls_planes", 10), ("mt_layernorm_bwd_rows_sums_sparse", 13)])
def test_entry_point_is_declared_and_bound(name, nparams):
    params = declared_params(name)
    assert params[-1] == "void* stream"                          # a launching entry point: csrc/gen_plan.py gives it a recording thunk
    assert name in L.LAUNCHES and len(L.LAUNCHES[name]) == len(params) == nparams
    hdr = header_text()
    decl = hdr[:hdr.index("int " + name)]
    assert ":270-276" in decl[decl.rindex("/*"):]                # the reference lines it implements: the head reads x[:, 0]


def _model(training, attn_p=0.0, ff_p=0.0, dim=512):
    return types.SimpleNamespace(training=training, attn_dropout=attn_p, ff_dropout=ff_p, dim=dim, heads=8, dim_head=64)


MIN = tsf_planes.PRUNE_MIN_CLIPS


def test_default_prunes_from_the_measured_batch_up(monkeypatch):
    monkeypatch.delenv("MT_TSF_PRUNE_LAST", raising=False)
    assert MIN == 32
    for training in (True, False):
        assert tsf_planes.prune_last(_model(training), MIN) and tsf_planes.prune_last(_model(training), 4 * MIN)
        assert not tsf_planes.prune_last(_model(training), MIN - 1) and not tsf_planes.prune_last(_model(training), 1)
    monkeypatch.setenv("MT_TSF_PRUNE_LAST", "1")                               # asked for: at any batch
    assert tsf_planes.prune_last(_model(True), 1) and tsf_planes.prune_last(_model(False), MIN)
    monkeypatch.setenv("MT_TSF_PRUNE_LAST", "0")
    assert not tsf_planes.prune_last(_model(True), MIN) and not tsf_planes.prune_last(_model(False), 4 * MIN)


@pytest.mark.parametrize("flag", [None, "1"])
def test_full_rows_where_pruning_would_change_results_or_cannot_run(flag, monkeypatch):
    if flag is None:
        monkeypatch.delenv("MT_TSF_PRUNE_LAST", raising=False)
    else:
        monkeypatch.setenv("MT_TSF_PRUNE_LAST", flag)
    assert not tsf_planes.prune_last(_model(True, ff_p=0.1), MIN) and not tsf_planes.prune_last(_model(True, attn_p=0.1), MIN)
    assert tsf_planes.prune_last(_model(False, attn_p=0.1, ff_p=0.1), MIN)     # eval mode: nn.Dropout is the identity
    # rows wider than 512 columns: the sparse-residual LayerNorm backward refuses them, so the full-row sequence (which has a
    # wide-row branch) runs
    assert tsf_planes.prune_last(_model(True, dim=512), MIN) and not tsf_planes.prune_last(_model(True, dim=528), MIN)
    assert not tsf_planes.prune_last(_model(False, dim=1024), MIN)
