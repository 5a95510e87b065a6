"""Learned-reward DrQ on the MI355X path: the learner labels rewards with a reward classifier at update time, as the
reference's VICE agent does (serl_launcher/agents/continuous/vice.py:546,594), and the classifier keeps training on goal
frames against the replay store's next-frames.  Alternating the two calls gives the VICE loop:

    classifier, loss, acc = train_step(classifier, {goal frames: 1, replay next-frames: 0}, key)
    agent, info = agent.update_high_utd(next(iterator), utd_ratio=1)       # rewards = sigmoid(classifier(next_obs)) >= 0.5
    print(info["vice_rewards"])                                            # the mean label of the batch (vice.py:609)

Both run on one stream, so each update reads the classifier the step before it left.  The classifier is given the agent's
frozen trunk: a label then costs the classifier's head on trunk features the update holds anyway (reward_label_mode
"features").  Not built: VICEAgent's own update_vice with mixup, label smoothing and gradient penalty.

    python examples/learner_vice_synthetic.py --steps 30 --batch_size 64 --size 64
"""
import argparse
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _Sp:
    def __init__(self, shape):
        self.shape = shape


class _Obs:
    def __init__(self, keys, H, W, S):
        self.spaces = {k: _Sp((1, H, W, 3)) for k in keys}
        self.spaces["state"] = _Sp((1, S))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=30, help="learner iterations (one classifier step + critic_actor_ratio agent updates each)")
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--size", type=int, default=64, help="image height and width")
    ap.add_argument("--transitions", type=int, default=600)
    ap.add_argument("--goal_frames", type=int, default=64)
    ap.add_argument("--critic_actor_ratio", type=int, default=2)
    ap.add_argument("--state_dim", type=int, default=24)
    ap.add_argument("--act_dim", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    from serl_amd import jaxrng as J
    from serl_amd.data.data_store import MemoryEfficientReplayBufferDataStore
    from serl_amd.networks.reward_classifier import Classifier, train_step
    from serl_amd.utils import init as pinit
    from serl_amd.utils.launcher import make_drq_agent
    from serl_amd.utils.synthetic import transition_stream

    keys, H, W, S, A, B = ("front", "wrist"), args.size, args.size, args.state_dim, args.act_dim, args.batch_size
    dev = torch.device("cuda", 0)
    store = MemoryEfficientReplayBufferDataStore(_Obs(keys, H, W, S), _Sp((A,)), args.transitions + 10, image_keys=keys)
    store.seed(args.seed)
    for tr in itertools.islice(transition_stream(keys, H, W, 3, 1, S, A, 50, 7), args.transitions):
        store.insert(tr)
    # goal frames: what success looks like (synthetic: brighter than anything in the store)
    g = torch.Generator().manual_seed(args.seed)
    goal = {k: torch.randint(160, 256, (args.goal_frames, 1, H, W, 3), dtype=torch.uint8, generator=g).to(dev) for k in keys}

    sample_obs = {k: np.zeros((1, H, W, 3), np.uint8) for k in keys}
    sample_obs["state"] = np.zeros((1, S), np.float32)
    agent = make_drq_agent(args.seed, sample_obs, np.zeros((A,), np.float32), image_keys=keys, encoder_type="resnet-pretrained",
                           batch_size=B)
    classifier = Classifier(keys, H, W, max_batch=B, trainable=True)
    for leaf, v in pinit.init_classifier(len(keys), H, W, args.seed).items():
        classifier.set(leaf, v)
    for leaf in (k for k in agent.core.leaves if k.startswith("trunk/")):      # one frozen trunk for both
        classifier.set(leaf, agent.core.get("params", leaf))
    agent.set_reward_classifier(classifier)
    print(f"reward_label_mode = {agent.reward_label_mode}")

    half = B // 2
    labels = torch.cat([torch.ones(half), torch.zeros(B - half)]).to(dev)
    rng = J.prngkey(args.seed)
    it = store.get_iterator(sample_args={"batch_size": B, "pack_obs_and_next_obs": True, "lazy": True})
    for step in range(args.steps):
        # classifier: goal frames positive, the store's next-frames negative (train_reward_classifier.py:122-137)
        pos = torch.randint(0, args.goal_frames, (half,), generator=g).to(dev)
        neg = store.gather(store.sample_indices(B - half))["observations"]
        data = {k: torch.cat([goal[k][pos], neg[k][:, 1:2]]) for k in keys}
        rng, key = J.split(rng)
        classifier, loss, acc = train_step(classifier, {"data": data, "labels": labels}, key)
        # agent: labelled updates (vice.py:546,594)
        for _ in range(args.critic_actor_ratio - 1):
            agent, _ = agent.update_critics(next(it))
        agent, info = agent.update_high_utd(next(it), utd_ratio=1)
        print(f"step {step:4d}  classifier loss {float(loss):.4f} acc {float(acc):.3f}  vice_rewards {info['vice_rewards']:.3f}  "
              f"critic_loss {info['critic']['critic_loss']:.4f}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
