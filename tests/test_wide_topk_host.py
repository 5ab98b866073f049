"""Rank lists past 64 columns, what needs no GPU: the limits and their messages, the loop's refusal of a cut-off nobody can
serve, the models' signatures, the header's new exports."""
import ctypes
import inspect

import pytest
import torch

from chaorec_amd import _lib, arg_parser, ops, ops_wide, ranking, registry
from chaorec_amd import Model as M
from chaorec_amd import train_and_evaluate as tae


def test_limits_are_one_number():
    assert ops_wide.WIDE_K == tae.MAX_TOPK == 1024 and ops_wide.NARROW_K == 64
    assert ops.score_topk_wide is ops_wide.score_topk_wide and "ops_wide" in ops._FAMILY_MODULES


def test_score_topk_beyond_1024_names_the_limit():
    ue, ie = torch.zeros(4, 8), torch.zeros(2000, 8)
    with pytest.raises(ValueError, match="1024"):
        ops.score_topk(ue, ie, None, 1e-6, 1025)
    with pytest.raises(ValueError, match="1024"):
        ranking.gene_ranklist(torch.zeros(2004, 8), 4, 2000, None, topk=1025)
    # up to the limit the call reaches the device check: there is no CPU route, wide or narrow
    for K in (50, 65, 1024):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.score_topk(ue, ie, None, 1e-6, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rows_topk(torch.zeros(2, 300), 100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rows_topk(torch.zeros(2, 300), 50)


def test_range_length_follows_the_staging_cap():
    assert ops_wide.WIDE_STAGING_BYTES == 512 << 20
    assert ops_wide.wide_range_users(15208) == (512 << 20) // (4 * 15208)
    assert ops_wide.wide_range_users(1300, 7 * 4 * 1300) == 7 and ops_wide.wide_range_users(1300, 7 * 4 * 1300 - 1) == 6
    assert ops_wide.wide_range_users(10 ** 9, 16) == 1          # never zero users


class _NoEpoch:
    """A loader the loop must not reach."""

    def __iter__(self):
        raise AssertionError("an epoch began")

    def __len__(self):
        raise AssertionError("an epoch began")


@pytest.mark.parametrize("trains", [True, False])
def test_loop_refuses_a_cut_off_past_1024_before_any_epoch(trains):
    class Model(torch.nn.Module):
        def gene_ranklist(self, topk=50, to_cpu=True):
            raise AssertionError("ranked")

    name = "LightGCN" if trains else "BSPM"
    assert registry.spec_of(name).trains is trains
    with pytest.raises(ValueError, match="1024"):
        tae.train_and_evaluate(Model(), _NoEpoch(), [[0, 1]], [[0, 1]], None, 3, model_name=name, topk=(20, 1025))


def test_loop_asks_for_the_columns_it_evaluates():
    calls = []

    class Model:
        def gene_ranklist(self, **kw):
            calls.append(kw)

    for kmax, on_device in ((20, True), (50, True), (50, False), (51, True), (100, False), (1024, True)):
        tae._rank_list(Model(), kmax, on_device)
    assert calls == [{"to_cpu": False}, {"to_cpu": False}, {}, {"topk": 51, "to_cpu": False}, {"topk": 100},
                     {"topk": 1024, "to_cpu": False}]


def test_every_registered_model_takes_topk():
    classes = [v for v in vars(M).values() if inspect.isclass(v) and hasattr(v, "gene_ranklist")]
    assert len(classes) == len(registry.MODELS) == 51
    for cls in classes:
        p = inspect.signature(cls.gene_ranklist).parameters
        assert "topk" in p and p["topk"].default == 50 and "to_cpu" in p, cls.__name__


def test_header_declares_the_new_exports():
    assert _lib.ABI_VERSION == 16
    res, args = _lib.SIGNATURES["chaorec_score_rows_f32"]
    assert res is ctypes.c_int and len(args) == 14 and args[5] is ctypes.c_int64 and args[12] is ctypes.c_size_t
    res, args = _lib.SIGNATURES["chaorec_rows_topk_wide_f32"]
    assert res is ctypes.c_int and len(args) == 9 and args[3] is ctypes.c_int64 and args[4] is ctypes.c_int32
    res, args = _lib.SIGNATURES["chaorec_rank_metrics_wide_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    assert not {"chaorec_score_rows_f32", "chaorec_rows_topk_wide_f32"} & _lib.INT_VALUE_EXPORTS       # statuses, checked by load()
    assert "topk_wide.hip" in _lib.SOURCES


def test_topk_flag_states_the_limit():
    assert "1024" in arg_parser.build_parser().format_help()
