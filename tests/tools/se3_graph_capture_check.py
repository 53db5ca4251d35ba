"""Run in its OWN process by tests/test_augmentation.py::test_augmentation_then_voxelizer_captured_into_a_hip_graph (stream capture
is process-wide state; a capture that goes wrong takes the process with it, not the test session).

Se3Augmentation -> voxelize_images (the augmented clouds are what the agent voxelizes) captured into ONE graph after eager
warm-up, then replayed while new clouds, poses, gripper poses and actions are written IN PLACE into the tensors the graph reads.
Both ops are deterministic, so after every replay the actions, the attempt info, every cloud, every pose and the grid equal, bit
for bit, an eager call made at the rng_state the replay started from; the replay advanced the offset by one (the in-place add is
part of the graph), and two replays on the same inputs draw different perturbations.  Prints GRAPH_OK on success."""
import faulthandler
import os
import sys

faulthandler.enable()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import se3_cases as sc  # noqa: E402
from manigaussian_amd import Se3Augmentation, voxelize_images  # noqa: E402

dev = torch.device("cuda:0")
B, CAMS, H, W, V = 2, 2, 16, 16, 20
SPEC = ("graph", B, H, W, CAMS, "one", [10, 15, 45], 0.125, "")


def stage(msg):
    print("stage:", msg, flush=True)


def inputs(seed):
    inp, _ = sc.make_inputs(SPEC, seed)
    t = torch.from_numpy
    rgb = [torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed + i)) for i in range(CAMS)]
    return [t(p) for p in inp["pcd"]] + [t(p) for p in inp["pose"]] + rgb + \
        [t(inp["gripper"]), t(inp["action_trans"]), t(inp["action_rot_grip"])]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu()


m = Se3Augmentation(sc.trans_aug_tensor(0.125), [10.0, 15.0, 45.0], sc.ROT_AUG_RESOLUTION, sc.VOXEL_SIZE, sc.ROT_RESOLUTION)
m = m.to(dev).manual_seed(5)
bounds = torch.tensor([sc.SCENE_BOUNDS], device=dev)
held = [x.to(dev).clone() for x in inputs(100)]


def step():
    pcd, pose, rgb = held[:CAMS], held[CAMS:2 * CAMS], held[2 * CAMS:3 * CAMS]
    trans, rot, new_pcd, new_pose = m(pcd, pose, held[-3], held[-2], held[-1], bounds)
    grid = voxelize_images(new_pcd, rgb, bounds, V)
    return [trans, rot, m.last_info] + new_pcd + new_pose + [grid]


side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    for _ in range(2):
        step()
torch.cuda.current_stream().wait_stream(side)
torch.cuda.synchronize()
assert m.rng_state.tolist() == [5, 2]
stage("warm-up done")
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    outs = step()
torch.cuda.synchronize()
m.rng_state.copy_(torch.tensor([5, 2]))  # (whatever the capture did to the buffer: the replays start from a known state)
stage("captured")
previous = None
for n, seed in enumerate((100, 101, 102, 102)):
    for dst, src in zip(held, inputs(seed)):
        dst.copy_(src.to(dev))
    start = m.rng_state.clone()
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in outs]
    assert m.rng_state.tolist() == [5, 2 + n + 1], f"the replay left rng_state at {m.rng_state.tolist()}"
    m.rng_state.copy_(start)
    eager = step()
    torch.cuda.synchronize()
    assert m.rng_state.tolist() == [5, 2 + n + 1]
    for i, (g, e) in enumerate(zip(got, eager)):
        assert torch.equal(bits(g), bits(e)), f"seed {seed}: output {i} of the replay differs from the eager call"
    print(f"seed {seed}: attempts {got[2].tolist()}, actions {got[0].tolist()}, occupied voxels {int(got[-1][..., -1].sum())}")
    assert int(got[2][0]) >= 0, "the constructed inputs were not accepted"
    if seed == 102 and previous is not None:
        assert not torch.equal(bits(got[3]), bits(previous[3])), "two replays on the same inputs drew the same perturbation"
    previous = got if seed == 102 else None
stage("replays equal the eager calls bit for bit, and every replay drew afresh")
print("GRAPH_OK")
