"""Reward-classifier training (examples/async_cable_route_drq/train_reward_classifier.py; the same file in
async_bin_relocation_fwbw_drq) on gfx950: positive / negative demos into the HBM data stores, then the reference's loop --
B/2 positives (next_observations) and B/2 negatives (observations) per epoch, random crop, train_step -- and a flax
checkpoint that load_classifier_func reads.  The reference's flags are kept; the robot environment is not needed: the
observation space comes from the first demo.

    python examples/train_reward_classifier.py --positive_demo_paths pos.pkl --negative_demo_paths neg.pkl \
        --classifier_ckpt_path ckpt --batch_size 256 --num_epochs 100
    python examples/train_reward_classifier.py --synthetic [--timing_steps 200]

--synthetic builds pos / neg demos from serl_amd/utils/synthetic.py (2 cameras, 128x128) and a random ResNet-10 pickle, runs
the loop, then times the train step and the frozen trunk alone over the same n_cam x B images.
"""
import argparse
import itertools
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore, populate_data_store  # noqa: E402
from serl_amd.networks.reward_classifier import train_reward_classifier, train_step  # noqa: E402


class _Sp:
    def __init__(self, shape):
        self.shape = shape


class _Obs:
    def __init__(self, spaces):
        self.spaces = spaces


def _space_of(demo_path):
    with open(demo_path, "rb") as f:
        t = pickle.load(f)[0]
    obs = t["observations"]
    return _Obs({k: _Sp(np.shape(v)) for k, v in obs.items()}), _Sp(np.shape(t["actions"]))


def _synthetic(args):
    from serl_amd.utils import init as pinit
    from serl_amd.utils.synthetic import transition_stream
    keys, H = ("front", "wrist"), args.size
    d = tempfile.mkdtemp(prefix="classifier_demos_")
    paths = []
    for j, name in enumerate(("pos", "neg")):
        p = os.path.join(d, f"{name}.pkl")
        with open(p, "wb") as f:
            pickle.dump(list(itertools.islice(transition_stream(keys, H, H, 3, 1, 7, 7, 100, 11 + j), args.demos)), f)
        paths.append([p])
    pkl = os.path.join(d, "resnet10_params.pkl")
    from serl_amd.agents.flax_tree import _trunk_paths
    tree = {}
    for leaf, sub in _trunk_paths().items():
        t = tree
        for s in sub[:-1]:
            t = t.setdefault(s, {})
        t[sub[-1]] = pinit.init_trunk(0)[leaf].reshape(pinit.trunk_shapes()[leaf])
    with open(pkl, "wb") as f:
        pickle.dump(tree, f)
    return paths[0], paths[1], pkl, os.path.join(d, "ckpt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positive_demo_paths", action="append", default=None, help="paths to positive demos")
    ap.add_argument("--negative_demo_paths", action="append", default=None, help="paths to negative demos")
    ap.add_argument("--classifier_ckpt_path", default=".", help="Path to classifier checkpoint")
    ap.add_argument("--batch_size", type=int, default=256, help="Batch size for training")
    ap.add_argument("--num_epochs", type=int, default=100, help="Number of epochs for training")
    ap.add_argument("--pretrained_encoder_path", default="./resnet10_params.pkl")
    ap.add_argument("--synthetic", action="store_true", help="synthetic demos and encoder; then time the step")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--demos", type=int, default=600)
    ap.add_argument("--timing_steps", type=int, default=200)
    args = ap.parse_args()
    pos_paths, neg_paths, enc_path, ckpt = args.positive_demo_paths, args.negative_demo_paths, args.pretrained_encoder_path, \
        args.classifier_ckpt_path
    if args.synthetic:
        pos_paths, neg_paths, enc_path, ckpt = _synthetic(args)
    obs_space, act_space = _space_of(pos_paths[0])
    image_keys = [k for k in obs_space.spaces if "state" not in k]   # train_reward_classifier.py:66
    pos_buffer = populate_data_store(MemoryEfficientReplayBufferDataStore(obs_space, act_space, capacity=10000, image_keys=image_keys),
                                     pos_paths)
    neg_buffer = populate_data_store(MemoryEfficientReplayBufferDataStore(obs_space, act_space, capacity=10000, image_keys=image_keys),
                                     neg_paths)
    print(f"failed buffer size: {len(neg_buffer)}")
    print(f"success buffer size: {len(pos_buffer)}")
    classifier, _ = train_reward_classifier(pos_buffer, neg_buffer, image_keys, batch_size=args.batch_size,
                                            num_epochs=args.num_epochs, classifier_ckpt_path=ckpt,
                                            pretrained_encoder_path=enc_path)
    print(f"checkpoint: {ckpt}/checkpoint_{args.num_epochs}")
    if not args.synthetic:
        return

    # timing: train_step on device-resident batches (the sampling and crop are not what is timed), then the trunk alone
    B, H, W = args.batch_size, classifier.H, classifier.W
    dev = torch.device("cuda", 0)
    frames = [torch.randint(0, 256, (len(image_keys), B, 1, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(4)]
    data = [{k: f[i] for i, k in enumerate(image_keys)} for f in frames]   # the cameras back to back, as the loop's batches
    labels = torch.cat([torch.ones(B // 2), torch.zeros(B // 2)]).to(dev)
    keys = [np.array([0, i], np.uint32) for i in range(8)]
    for i in range(20):
        classifier, loss, acc = train_step(classifier, {"data": data[i % 4], "labels": labels}, keys[i % 8])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.timing_steps):
        classifier, loss, acc = train_step(classifier, {"data": data[i % 4], "labels": labels}, keys[i % 8])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.timing_steps
    print(f"classifier train step  B={B} {len(image_keys)}x{H}x{W}: {ms:.3f} ms/step ({1e3 / ms:.0f} steps/s)  "
          f"loss {float(loss):.4f} accuracy {float(acc):.4f}")
    from serl_amd.agents.core import AgentCore
    core = AgentCore(n_cam=len(image_keys), H=H, W=W, state_dim=7, act_dim=7, batch=B)
    frames = torch.randint(0, 256, (len(image_keys) * B, H, W, 3), dtype=torch.uint8, device=dev)
    for _ in range(20):
        core.trunk_forward(frames)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.timing_steps):
        core.trunk_forward(frames)
    torch.cuda.synchronize()
    tms = (time.perf_counter() - t0) * 1e3 / args.timing_steps
    print(f"trunk    {len(image_keys) * B} images {H}x{W}: {tms:.3f} ms/pass  (train step = trunk + {ms - tms:.3f} ms)")


if __name__ == "__main__":
    main()
