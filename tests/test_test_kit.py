"""The test kit's own tests, none of which needs a GPU: numerics.py (bits, same_bits, rel_err, spy), child.py (the graph tools'
runner, against throw-away children that import nothing of the project) and the comparison of tests/tools/_graph.py."""
import importlib.util
import os
import types

import pytest
import torch

from child import run_graph_tool
from numerics import rel_err, same_bits, spy

_spec = importlib.util.spec_from_file_location("_graph", os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "_graph.py"))
_graph = importlib.util.module_from_spec(_spec)   # (by its path: the tools' directory stays off this session's sys.path)
_spec.loader.exec_module(_graph)


def nan32(payload):
    return torch.tensor([0x7FC00000 | payload], dtype=torch.int32).view(torch.float32)


# ---- same_bits ------------------------------------------------------------------------------------------------------------------
def test_same_bits_tells_the_zeros_apart():
    assert not same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert same_bits(torch.tensor([-0.0]), torch.tensor([-0.0]))


def test_same_bits_compares_nans_by_payload():
    assert same_bits(nan32(1), nan32(1))
    assert not same_bits(nan32(1), nan32(2))
    assert same_bits(torch.tensor([float("nan"), 1.0]), torch.tensor([float("nan"), 1.0]))


def test_same_bits_asks_for_the_same_dtype_and_shape():
    x = torch.arange(6, dtype=torch.float32)
    assert not same_bits(x, x.double())
    assert not same_bits(x.reshape(2, 3), x.reshape(3, 2))
    assert same_bits(x.reshape(2, 3), x.clone().reshape(2, 3))


def test_same_bits_reads_a_view_in_its_own_order():
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    view = x.t()
    assert not view.is_contiguous() and same_bits(view, view.contiguous())
    assert not same_bits(view, x.reshape(4, 3))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.bool, torch.uint8, torch.float64, torch.float16])
def test_same_bits_takes_integer_bool_and_other_float_tensors(dtype):
    a = torch.tensor([0, 1, 1, 0, 1]).to(dtype)
    b = a.clone()
    assert same_bits(a, b) and same_bits(a[0], b[0])   # (a scalar tensor as well)
    b[2] = 0
    assert not same_bits(a, b)


# ---- rel_err --------------------------------------------------------------------------------------------------------------------
def test_rel_err_is_relative_to_the_largest_truth_and_absolute_for_a_zero_truth():
    truth = torch.tensor([1.0, -4.0, 2.0])
    assert rel_err(truth + torch.tensor([0.0, 0.0, 0.5]), truth) == 0.125
    assert rel_err(torch.tensor([0.0, 0.25]), torch.zeros(2)) == 0.25
    assert rel_err(torch.zeros(2), torch.zeros(2)) == 0.0


def test_rel_err_works_in_float64_on_the_cpu():
    truth = torch.tensor([1.0], dtype=torch.float64, requires_grad=True)
    got = torch.tensor([1.0 + 2.0 ** -20], dtype=torch.float32)
    assert rel_err(got, truth) == 2.0 ** -20   # (exact in float64; float32 against float64, and a tensor that asks for a gradient)


# ---- same_step ------------------------------------------------------------------------------------------------------------------
def step_results():
    g = torch.Generator().manual_seed(1)
    return [torch.rand(3, 8, 8, generator=g), torch.rand(5, generator=g), torch.randn(100, 3, generator=g)]


def test_same_step_allows_a_gradient_the_atomic_order_and_no_more():
    want = step_results()
    top = want[2].abs().max().item()
    at = int(want[2].abs().argmin())   # (the smallest element: the sum rounds least there)
    for factor, passes in ((1.9e-5, True), (2.1e-5, False)):
        got = [t.clone() for t in want]
        got[2].view(-1)[at] += factor * top
        if passes:
            _graph.same_step(got, want, 2, "kit")
        else:
            with pytest.raises(AssertionError, match="kit: gradients differ"):
                _graph.same_step(got, want, 2, "kit")


def test_same_step_sees_one_bit_of_an_exact_value():
    want = step_results()
    got = [t.clone() for t in want]
    _graph.same_step(got, want, 2, "kit")
    got[1].view(torch.int32)[3] ^= 1
    with pytest.raises(AssertionError, match="kit: value 1 differs"):
        _graph.same_step(got, want, 2, "kit")
    with pytest.raises(AssertionError):
        _graph.same_step(got[:2], want, 2, "kit")   # (a result is missing)


# ---- run_graph_tool -------------------------------------------------------------------------------------------------------------
def child(tmp_path, body):
    path = tmp_path / "child.py"
    path.write_text(body)
    return str(path)


def test_runner_passes_a_child_that_exits_0_with_graph_ok(tmp_path):
    run_graph_tool(child(tmp_path, "import sys\nprint('stage: got', sys.argv[1:], flush=True)\nprint('GRAPH_OK')\n"), "a", "b")


def test_runner_fails_a_child_without_graph_ok(tmp_path):
    with pytest.raises(AssertionError, match="exit 0"):
        run_graph_tool(child(tmp_path, "print('stage: nothing checked', flush=True)\n"))


def test_runner_fails_a_child_that_exits_1_after_graph_ok(tmp_path):
    with pytest.raises(AssertionError, match="exit 1"):
        run_graph_tool(child(tmp_path, "import sys\nprint('GRAPH_OK', flush=True)\nsys.exit(1)\n"))


def test_runner_ends_a_child_at_its_limit_and_shows_how_far_it_came(tmp_path):
    body = "import sys, time\nprint('stage: captured', flush=True)\nprint('on stderr', file=sys.stderr, flush=True)\ntime.sleep(30)\nprint('GRAPH_OK')\n"
    with pytest.raises(AssertionError) as e:
        run_graph_tool(child(tmp_path, body), limit=1)
    message = str(e.value)
    assert "exit 124" in message and "stage: captured" in message and "on stderr" in message and "GRAPH_OK" not in message


# ---- spy ------------------------------------------------------------------------------------------------------------------------
def library():
    return types.SimpleNamespace(add=lambda a, b: a + b, neg=lambda a: -a)


def test_spy_records_the_arguments_and_returns_what_the_function_returns():
    lib, order = library(), []
    seen = spy(lib, ["add", "neg"], on_call=lambda name, a: order.append(name))
    assert seen == {}
    assert lib.add(1, 2) == 3 and lib.neg(5) == -5 and lib.add(3, 4) == 7
    assert seen == {"add": [(1, 2), (3, 4)], "neg": [(5,)]} and order == ["add", "neg", "add"]
    assert len(seen["add"]) == 2


def test_spy_with_a_monkeypatch_is_undone_with_it():
    lib = library()
    real = lib.add
    with pytest.MonkeyPatch.context() as mp:
        seen = spy(lib, ["add"], mp)
        assert lib.add is not real and lib.add(1, 1) == 2 and seen["add"] == [(1, 1)]
    assert lib.add is real and lib.add(2, 2) == 4 and seen["add"] == [(1, 1)]
