"""That the Conv3d families' shared test harness (tests/conv_family.py, tests/conv_cases.py) can fail: fake results against the real
references, on the CPU."""
import ctypes

import pytest
import torch

import conv_family as cf
import pointwise_cases as pc

CASE = "odd"


def _truths():
    r = pc.reference(CASE)
    return {q: r[q + "64"].float() for q in pc.quantities(CASE)}


def _moved(q, factor):
    """The float32 truths with the largest element of q moved by factor x its bound."""
    r, got = pc.reference(CASE), _truths()
    at = r[q + "64"].abs().argmax()
    got[q].view(-1)[at] += factor * pc.bound(r["ref_err"][q], r[q + "64"])
    return got


def test_the_comparison_passes_the_rounded_truth_and_half_a_bound(capsys):
    cf.compare(pc, CASE, _truths())
    assert capsys.readouterr().out.count(" err ") == len(pc.quantities(CASE))
    for q in pc.quantities(CASE):
        cf.compare(pc, CASE, _moved(q, 0.5))


@pytest.mark.parametrize("q", pc.quantities(CASE))
def test_the_comparison_fails_on_one_element_moved_by_twice_its_bound(q):
    with pytest.raises(AssertionError) as failure:
        cf.compare(pc, CASE, _moved(q, 2.0))
    case, fails = failure.value.args[0]
    assert case == CASE and [f[0] for f in fails] == [q] and fails[0][1] > fails[0][2]


def test_the_comparison_fails_on_a_wrong_shape_and_on_a_float64_result():
    got = _truths()
    got["dw"] = got["dw"][..., 0]
    with pytest.raises(AssertionError):
        cf.compare(pc, CASE, got)
    got = _truths()
    got["y"] = got["y"].double()
    with pytest.raises(AssertionError):
        cf.compare(pc, CASE, got)


def test_the_module_comparison_fails_beyond_sixteen_yardsticks(capsys):
    truth = {"y": torch.tensor([1.0, -4.0], dtype=torch.float64)}
    torchs = {"y": truth["y"] + torch.tensor([0.0, 4e-6], dtype=torch.float64)}   # a yardstick of 1e-6 of 4
    bound = 16 * 1e-6 * 4

    def routed(factor):
        return {"y": truth["y"] + torch.tensor([factor * bound, 0.0], dtype=torch.float64)}
    cf.compare_modules("stem", "torch's fp32 path", truth, torchs, routed(0.5))
    assert capsys.readouterr().out.startswith("stem y: err 3.200e-05, bound 6.400e-05 (torch's fp32 path 1.00e-06 of 4.000e+00)")
    with pytest.raises(AssertionError):
        cf.compare_modules("stem", "torch's fp32 path", truth, torchs, routed(2.0))
    cf.compare_modules("stem", "torch's fp32 path", truth, truth, routed(0.0))   # a yardstick of 0: the floor
    with pytest.raises(AssertionError):
        cf.compare_modules("stem", "torch's fp32 path", truth, truth, {"y": truth["y"] + 16.5 * 2.0 ** -23 * 4})


def test_same_bits_tells_the_sign_of_zero_and_the_last_mantissa_bit():
    a = torch.tensor([0.0, 1.0, -3.5])
    assert cf.same_bits(a, a.clone())
    assert a[0] == -a[0] and not cf.same_bits(a, torch.tensor([-0.0, 1.0, -3.5]))
    assert not cf.same_bits(a, torch.nextafter(a, torch.full_like(a, 9.0)))
    assert not cf.same_bits(a, a.double()) and not cf.same_bits(a, a.view(3, 1))


def test_the_watched_arguments_are_where_the_header_names_them():
    """The positions the families' tests hard-coded before the lookup by name: a[7:10], a[10:14], a[12:16]."""
    assert cf.backward_positions(cf.FAMILIES["pointwise"]) == {"mgs_pointwise_backward": (7, 8, 9)}
    assert cf.backward_positions(cf.FAMILIES["narrow"]) == {"mgs_narrow_conv3d_backward": (10, 11, 12, 13)}
    assert cf.backward_positions(cf.FAMILIES["dense"]) == {"mgs_dense_conv3d_backward": (12, 13, 14, 15)}
    assert cf.backward_positions(cf.FAMILIES["conv3d"]) == {"mgs_conv3d_backward_data": (), "mgs_conv3d_backward_weight": ()}
    assert cf.parameters("mgs_pointwise_backward")[7:10] == ["dx", "dw", "db"] and cf.parameters("mgs_abi_version") == []


def test_count_calls_records_what_is_given(monkeypatch):
    fam = cf.FAMILIES["narrow"]
    calls = cf.count_calls(monkeypatch, fam)
    args = [0] * 17
    args[10], args[13] = cf.FAKE, cf.FAKE + 8   # dx and a misaligned workspace: refused before any launch
    assert cf._lib.lib().mgs_narrow_conv3d_backward(*args) == cf._lib.MGS_ERR_INVALID_ARG
    assert calls == [("backward", True, False, False, True)]


def test_the_expected_calls_of_the_families():
    need = (False, True, False)
    assert cf.FAMILIES["pointwise"].expected("odd", need) == [("forward",), ("backward", False, True, False)]
    assert cf.FAMILIES["pointwise"].expected("no_bias", (False, False, True)) == [("forward",)]
    assert cf.FAMILIES["narrow"].expected("odd", need) == [("forward",), ("backward", False, True, False, True)]
    assert cf.FAMILIES["dense"].expected("odd_k3", need) == [("forward",), ("backward", False, True, False, False)]
    assert cf.FAMILIES["conv3d"].expected("odd_s1", need) == [("forward",), ("backward_weight",)]
    assert cf.FAMILIES["conv3d"].expected("up_odd", (True, True, False)) == [("backward_data",), ("forward",), ("backward_weight",)]


def _entry(op_q3, torch_q1, benchmark):
    side = lambda q1: {"median_us": q1 + 1.0, "q1_us": q1, "q3_us": q1 + 2.0}   # noqa: E731
    sides = {"op": {"median_us": op_q3 - 1.0, "q1_us": op_q3 - 2.0, "q3_us": op_q3}, "torch": side(torch_q1)}
    if benchmark is not None:
        sides["torch_benchmark"] = benchmark if isinstance(benchmark, dict) else side(benchmark)
    return {p: {f: dict(sides) for f in ("eager", "graph")} for p in ("forward", "forward_backward")}


def test_op_wins_is_strict_unless_told_that_the_benchmark_side_may_be_missing():
    assert cf.op_wins(_entry(10.0, 11.0, 12.0)) and not cf.op_wins(_entry(10.0, 11.0, 9.0))   # (the faster torch setting decides)
    assert not cf.op_wins(_entry(10.0, 10.0, 12.0))
    for missing in (None, {"status": "did not finish"}):
        with pytest.raises(KeyError):
            cf.op_wins(_entry(10.0, 11.0, missing))
        assert cf.op_wins(_entry(10.0, 11.0, missing), benchmark_may_be_missing=True)
        assert not cf.op_wins(_entry(10.0, 9.0, missing), benchmark_may_be_missing=True)
    assert not cf.op_wins(_entry(10.0, 11.0, 9.0), benchmark_may_be_missing=True)


def test_check_abi_fails_on_one_argument_too_many_and_on_a_wrong_size_type():
    cf.check_abi(cf.FAMILIES["dense"].names)
    for name in ("mgs_dense_conv3d_backward", "mgs_abi_version", "mgs_ledger_drain"):
        table = cf.ctypes_table()
        table[name] = (table[name][0], table[name][1] + [ctypes.c_int])
        with pytest.raises(AssertionError, match=name):
            cf.check_abi(table=table)
    table = cf.ctypes_table()
    table["mgs_pointwise_workspace_bytes"] = (ctypes.c_int, table["mgs_pointwise_workspace_bytes"][1])
    with pytest.raises(AssertionError, match="mgs_pointwise_workspace_bytes"):
        cf.check_abi(table=table)
    table = cf.ctypes_table()
    del table["mgs_selftest"]
    with pytest.raises(AssertionError, match="disagree"):
        cf.check_abi(table=table)
    with pytest.raises(AssertionError, match="mgs_no_such_entry"):
        cf.check_abi(("mgs_no_such_entry",))
