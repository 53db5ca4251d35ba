"""Run in its OWN process by tests/test_augmentation.py::test_augmentation_then_voxelizer_captured_into_a_hip_graph (stream capture
is process-wide state; a capture that goes wrong takes the process with it, not the test session).

Se3Augmentation -> voxelize_images (the augmented clouds are what the agent voxelizes) captured into ONE graph after eager
warm-up, then replayed while new clouds, poses, gripper poses and actions are written IN PLACE into the tensors the graph reads.
Both ops are deterministic, so after every replay the actions, the attempt info, every cloud, every pose and the grid equal, bit
for bit, an eager call made at the rng_state the replay started from; the replay advanced the offset by one (the in-place add is
part of the graph), and two replays on the same inputs draw different perturbations.  Prints GRAPH_OK on success."""
import _graph
import torch

import se3_cases as sc
from manigaussian_amd import Se3Augmentation, voxelize_images
from numerics import same_bits

dev = _graph.DEV
B, CAMS, H, W, V = 2, 2, 16, 16, 20
SPEC = ("graph", B, H, W, CAMS, "one", [10, 15, 45], 0.125, "")


def inputs(seed):
    inp, _ = sc.make_inputs(SPEC, seed)
    t = torch.from_numpy
    rgb = [torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed + i)) for i in range(CAMS)]
    return [t(p) for p in inp["pcd"]] + [t(p) for p in inp["pose"]] + rgb + \
        [t(inp["gripper"]), t(inp["action_trans"]), t(inp["action_rot_grip"])]


m = Se3Augmentation(sc.trans_aug_tensor(0.125), [10.0, 15.0, 45.0], sc.ROT_AUG_RESOLUTION, sc.VOXEL_SIZE, sc.ROT_RESOLUTION)
m = m.to(dev).manual_seed(5)
bounds = torch.tensor([sc.SCENE_BOUNDS], device=dev)
held = [x.to(dev).clone() for x in inputs(100)]


def step():
    pcd, pose, rgb = held[:CAMS], held[CAMS:2 * CAMS], held[2 * CAMS:3 * CAMS]
    trans, rot, new_pcd, new_pose = m(pcd, pose, held[-3], held[-2], held[-1], bounds)
    grid = voxelize_images(new_pcd, rgb, bounds, V)
    return [trans, rot, m.last_info] + new_pcd + new_pose + [grid]


_graph.warm_up(step)
assert m.rng_state.tolist() == [5, 2]
_graph.stage("warm-up done")
graph, outs = _graph.capture(step)
m.rng_state.copy_(torch.tensor([5, 2]))  # (whatever the capture did to the buffer: the replays start from a known state)
_graph.stage("captured")
previous = None
for n, seed in enumerate((100, 101, 102, 102)):
    for dst, src in zip(held, inputs(seed)):
        dst.copy_(src.to(dev))
    start = m.rng_state.clone()
    _graph.replay(graph)
    got = [o.clone() for o in outs]
    assert m.rng_state.tolist() == [5, 2 + n + 1], f"the replay left rng_state at {m.rng_state.tolist()}"
    m.rng_state.copy_(start)
    eager = step()
    torch.cuda.synchronize()
    assert m.rng_state.tolist() == [5, 2 + n + 1]
    _graph.equal_bits(got, eager, [f"output {i} of the replay" for i in range(len(got))], f"seed {seed}")
    print(f"seed {seed}: attempts {got[2].tolist()}, actions {got[0].tolist()}, occupied voxels {int(got[-1][..., -1].sum())}")
    assert int(got[2][0]) >= 0, "the constructed inputs were not accepted"
    if seed == 102 and previous is not None:
        assert not same_bits(got[3], previous[3]), "two replays on the same inputs drew the same perturbation"
    previous = got if seed == 102 else None
_graph.stage("replays equal the eager calls bit for bit, and every replay drew afresh")
_graph.ok()
