"""Cases, fixtures, bounds and the restatement shared by tests/test_encoder.py, tests/golden/make_golden_abn.py and
tests/tools/abn_graph_capture_check.py -- TEST INFRASTRUCTURE.

A fixture (tests/golden/abn/<case>.npz, arrays only) holds what ManiGaussian's own InPlaceABN (helpers/network_utils.py:219-231,
executed unmodified on a CPU) was given and gave for  y = residual + InPlaceABN(x),  loss = sum(y g):
  x, residual, g [B,C,D,H,W], weight, bias [C]: float32 (residual is absent in the case without a skip tensor);
  running_mean0, running_var0 [C] (case `eval` only): the running buffers the module normalises with;
  y64, dx64, dweight64, dbias64, running_mean64, running_var64: the float64 module's results -- the truth (the running buffers
  after ONE training forward from their initial 0 and 1; the eval case has y64 alone);
  ref_err [len(QUANTITIES)]: the float32 module's largest deviation from each truth over the truth's largest magnitude -- the
  yardsticks (0 where the case has no such quantity);
  seed [1]: the generator seed that produced the inputs (the first one without an element near the activation's kink).
"""
import importlib.util
import os

import numpy as np
import torch

from numerics import same_bits  # noqa: F401  (re-exported: the tests and the tools reach them through this module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "abn")
NAMES_FILE = os.path.join(GOLDEN_DIR, "stem_state_dict_names.txt")
REF_FILE = os.path.join(os.environ.get("MGS_REFERENCE_ROOT", "/root/reference"), "helpers", "network_utils.py")
FACTOR = 16.0              # tolerance = FACTOR x the reference's own float32 error (spatial_softmax_cases.FACTOR) ...
FLOOR = 2.0 ** -23         # ... and at least FACTOR x 2^-23, both relative to the truth's largest magnitude
REF_ERR_CEILING = 2e-4     # the generator refuses a case whose yardstick is looser than this
KINK = 1e-5                # |z64| below this: the element may take the other branch of the activation in any float32 run
EPS = 1e-5
MOMENTUM = 0.1
QUANTITIES = ("y", "dx", "dweight", "dbias", "running_mean", "running_var")

# name: B, C, D, H, W, the input's mean and std, the slope, and what else is special
CASES = {
    "tiny":         dict(shape=(2, 3, 2, 3, 4)),
    "odd":          dict(shape=(2, 5, 7, 9, 11)),                       # odd row length: the second row starts misaligned
    "batch3":       dict(shape=(3, 2, 6, 6, 6)),                        # statistics across batch entries
    "deep":         dict(shape=(1, 64, 2, 2, 2)),                       # the stem's smallest site at 12^3: 8 values per channel
    "offset":       dict(shape=(1, 4, 12, 12, 12), mean=37.5, std=0.05),   # variance cancellation
    "dead_channel": dict(shape=(2, 4, 3, 5, 7), dead=1),                # weight = bias = 0 in one channel: z == 0 everywhere there
    "relu":         dict(shape=(2, 3, 4, 5, 6), activation="relu"),     # InPlaceABN's 'relu': slope 0
    "no_residual":  dict(shape=(2, 3, 3, 4, 5), residual=False),
    "eval":         dict(shape=(2, 4, 3, 4, 5), training=False),        # running statistics, forward only
}
MAX_SEEDS = 20


def slope_of(case):
    return 0.0 if CASES[case].get("activation") == "relu" else 0.01


def make_inputs(case, seed):
    """{name: fp32 CPU tensor} from a generator seeded by `seed`."""
    c = CASES[case]
    B, C, D, H, W = c["shape"]
    g = torch.Generator().manual_seed(seed)
    t = {"x": torch.randn(B, C, D, H, W, generator=g) * c.get("std", 1.0) + c.get("mean", 0.0)}
    if c.get("residual", True):
        t["residual"] = torch.randn(B, C, D, H, W, generator=g)
    t["g"] = torch.randn(B, C, D, H, W, generator=g)
    t["weight"] = 1.0 + 0.5 * torch.randn(C, generator=g)
    t["bias"] = 0.3 * torch.randn(C, generator=g)
    if "dead" in c:
        t["weight"][c["dead"]] = 0.0
        t["bias"][c["dead"]] = 0.0
    if not c.get("training", True):
        t["running_mean0"] = 0.2 * torch.randn(C, generator=g)
        t["running_var0"] = 0.5 + torch.rand(C, generator=g)
    return t


def restatement(x, weight, bias, residual, slope, dtype, running=None, eps=EPS):
    """The reference's formula in plain torch ops, in `dtype`, on the device of x: (y, z, mean [C], unbiased variance [C]),
    differentiable towards x, weight, bias and residual.  running = (mean, var): eval mode.  z is the activation's argument.
    torch.where routes the gradient at z == 0 to the slope branch, as the activation's own backward does.  Stands where the
    reference cannot be (the GPU tests); pinned against the fixtures on the CPU."""
    xd = x.to(dtype)
    C = xd.size(1)
    n = xd.numel() // C
    view = (1, C, 1, 1, 1)
    if running is None:
        mean = xd.mean(dim=(0, 2, 3, 4))
        var = ((xd - mean.view(view)) ** 2).mean(dim=(0, 2, 3, 4))
        unbiased = var * (n / (n - 1)) if n > 1 else var
    else:
        mean, var = running[0].to(dtype), running[1].to(dtype)
        unbiased = var
    z = (xd - mean.view(view)) / torch.sqrt(var.view(view) + eps) * weight.to(dtype).view(view) + bias.to(dtype).view(view)
    y = torch.where(z > 0, z, z * slope)
    if residual is not None:
        y = residual.to(dtype) + y
    return y, z, mean, unbiased


def running_after_one_step(mean, unbiased, momentum=MOMENTUM):
    """The running buffers after one training forward from nn.BatchNorm3d's initial (0, 1)."""
    return momentum * mean, (1 - momentum) + momentum * unbiased


# ---- the reference -----------------------------------------------------------------------------------------------------------
def have_reference() -> bool:
    return os.path.isfile(REF_FILE)


_REF = []


def load_reference():
    """helpers/network_utils.py, unmodified."""
    if not _REF:
        spec = importlib.util.spec_from_file_location("_mgs_reference_network_utils", REF_FILE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _REF.append(mod)
    return _REF[0]


def _run(ref, case, t, dtype):
    c = CASES[case]
    m = ref.InPlaceABN(c["shape"][1], activation=c.get("activation", "leaky_relu")).to(dtype)
    with torch.no_grad():
        m.bn.weight.copy_(t["weight"])
        m.bn.bias.copy_(t["bias"])
        if "running_mean0" in t:
            m.bn.running_mean.copy_(t["running_mean0"])
            m.bn.running_var.copy_(t["running_var0"])
    m.train(c.get("training", True))
    x = t["x"].to(dtype).clone().requires_grad_(True)
    y = m(x)
    if "residual" in t:
        y = t["residual"].to(dtype) + y
    res = {"y": y.detach()}
    if c.get("training", True):
        (y * t["g"].to(dtype)).sum().backward()
        res.update(dx=x.grad, dweight=m.bn.weight.grad, dbias=m.bn.bias.grad, running_mean=m.bn.running_mean.clone(),
                   running_var=m.bn.running_var.clone())
        assert int(m.bn.num_batches_tracked) == 1
    return res


def near_kink(z64):
    return z64.abs() < KINK


def reference_case(case):
    """{array name: numpy array}: the fixture of `case`, computed from the reference; the first seed whose inputs have no element
    near the kink (outside a dead channel, where every element is AT it by construction)."""
    ref = load_reference()
    c = CASES[case]
    base = 3000 + 100 * list(CASES).index(case)
    for seed in range(base, base + MAX_SEEDS):
        t = make_inputs(case, seed)
        running = (t["running_mean0"], t["running_var0"]) if "running_mean0" in t else None
        z64 = restatement(t["x"], t["weight"], t["bias"], None, slope_of(case), torch.float64, running)[1]
        live = torch.ones(c["shape"][1], dtype=torch.bool)
        if "dead" in c:
            live[c["dead"]] = False
        if not bool(near_kink(z64)[:, live].any()):
            break
    else:
        raise AssertionError(f"{case}: no seed without an element near the kink")
    r32, r64 = _run(ref, case, t, torch.float32), _run(ref, case, t, torch.float64)
    out = {k: v.numpy() for k, v in t.items()}
    err = []
    for q in QUANTITIES:
        if q not in r64:
            err.append(0.0)
            continue
        out[q + "64"] = r64[q].numpy()
        mag = r64[q].abs().max().item()
        err.append((r32[q].double() - r64[q]).abs().max().item() / mag if mag > 0 else 0.0)
    assert max(err) <= REF_ERR_CEILING, (case, err)
    out["ref_err"] = np.asarray(err, dtype=np.float64)
    out["seed"] = np.asarray([seed], dtype=np.int64)
    return out


def fixture_path(case):
    return os.path.join(GOLDEN_DIR, case + ".npz")


_FIXTURES = {}


def load_fixture(case):
    """The committed fixture as {name: tensor}, loaded once and shared (do not modify); ref_err as {quantity: float}."""
    if case not in _FIXTURES:
        with np.load(fixture_path(case)) as z:
            f = {k: torch.from_numpy(z[k]) for k in z.files if k != "ref_err"}
            f["ref_err"] = dict(zip(QUANTITIES, z["ref_err"].tolist()))
        _FIXTURES[case] = f
    return _FIXTURES[case]


def bound(ref_err, truth):
    """Largest allowed |ours - truth|."""
    return max(FACTOR * ref_err, FACTOR * FLOOR) * truth.abs().max().item()


def stem_state_dict_names():
    with open(NAMES_FILE) as f:
        return f.read().split()
