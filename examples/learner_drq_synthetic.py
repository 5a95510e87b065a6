"""The learner loop of the reference's examples/async_drq_sim/async_drq_sim.py:183-311 on the MI355X path.  The actor
side is an in-process mock (a thread with a TrainerClient + QueuedDataStore that ships synthetic transitions, requests
"send-stats" and receives every published network) talking to the learner's TrainerServer through serl_amd.transport
-- the agentlace call pattern of the reference script (server.register_data_store / start / publish_network,
client.update / request / recv_network_callback); real ZeroMQ is used when pyzmq + lz4 are installed.

    python examples/learner_drq_synthetic.py --steps 200 --batch_size 256 --critic_actor_ratio 4

Only the import lines differ from the reference script: make_drq_agent / make_replay_buffer / concat_batches come
from serl_amd, `lazy=True` lets gather + concat + unpack + random-shift crop fuse into the update, and checkpoints
go through serl_amd.utils.checkpoint (flax's file layout).

Stopping and continuing:  --run_dir DIR --save_every N  saves the run state (the agent's checkpoint, state.rng included, plus a
snapshot of both replay stores) every N steps; the same command with  --resume  continues from the latest one: the demo store
is not filled again and the online store already holds what the actor had sent.

Publishing:  --publish sync  (default) is the reference's line, server.publish_network(agent.state.params): one blocking copy per
leaf, pickle, LZ4 and send on the training thread.  --publish snapshot  is server.publish_network(agent.snapshot): the server takes
the snapshot -- one kernel launch on the update stream --, the copy to pinned host memory and the encoding happen behind the
learner's back, a publisher that falls behind drops a network instead of stalling the learner, and parameters that have gone NaN
are never sent; with --checkpoint_path the checkpoints are then taken from a three-section snapshot too.
"""
import argparse
import itertools
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serl_amd.agents.drq import DrQAgent  # noqa: E402
from serl_amd.transport import QueuedDataStore, TrainerClient, TrainerServer, make_trainer_config  # noqa: E402
from serl_amd.utils.checkpoint import restore_run, save_checkpoint, save_run  # noqa: E402
from serl_amd.utils.launcher import make_drq_agent, make_replay_buffer  # noqa: E402
from serl_amd.utils.synthetic import transition_stream  # noqa: E402
from serl_amd.utils.train_utils import concat_batches  # noqa: E402

KEYS, H, W, S, A = ("front", "wrist"), 128, 128, 7, 4


class _Sp:
    def __init__(self, shape):
        self.shape = shape


class _Env:  # observation/action spaces of the PandaPickCubeVision env wrapped as in the reference (T = 1)
    class _Obs:
        spaces = {"front": _Sp((1, H, W, 3)), "state": _Sp((1, S)), "wrist": _Sp((1, H, W, 3))}
    observation_space, action_space = _Obs(), _Sp((A,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--critic_actor_ratio", type=int, default=4)
    ap.add_argument("--training_starts", type=int, default=1000)
    ap.add_argument("--checkpoint_path", default=None)
    ap.add_argument("--checkpoint_period", type=int, default=0)
    ap.add_argument("--log_period", type=int, default=20)
    ap.add_argument("--steps_per_update", type=int, default=30)      # async_drq_sim.py:60
    ap.add_argument("--port", type=int, default=5488)
    ap.add_argument("--run_dir", default=None, help="directory of the run state (save_run / restore_run)")
    ap.add_argument("--save_every", type=int, default=0, help="save the run state every N steps (needs --run_dir)")
    ap.add_argument("--resume", action="store_true", help="continue from the latest run state in --run_dir")
    ap.add_argument("--hidden", type=int, default=256,
                    help="width h of the critic's and the policy's MLPs (hidden_dims=[h, h]): a multiple of 64 in [64, 1024]")
    ap.add_argument("--critic_dims", type=int, nargs="+", default=None,
                    help="hidden_dims of the critic's MLP, 1 to 4 widths (multiples of 64 in [64, 1024]), e.g. 512 512 512: the critic "
                         "never leaves the learner; default [hidden, hidden]")
    ap.add_argument("--policy_dims", type=int, nargs="+", default=None,
                    help="hidden_dims of the policy's MLP, the network that is published to the actor; default [hidden, hidden]")
    ap.add_argument("--publish", choices=["sync", "snapshot"], default="sync",
                    help="sync: publish_network(agent.state.params) on the training thread; snapshot: publish_network(agent.snapshot)")
    ap.add_argument("--activation", choices=["tanh", "relu", "swish"], default="tanh",
                    help="activation of the critic's and the policy's MLPs (the launcher writes tanh)")
    ap.add_argument("--eval-every", dest="eval_every", type=int, default=0,
                    help="every K steps print the ensemble's mean Q on a demo batch and the mean log-prob of its actions "
                         "(agent.evaluate_batch: read-only for the agent; the extra sample advances the demo store's sampler)")
    ap.add_argument("--weight_decay", type=float, default=None,
                    help="weight_decay of all three optimizers (optax.adamw).  It decays the whole tree, the pretrained ResNet-10 "
                         "included, as in the reference -- not a recommendation: the agent then runs with a live trunk "
                         "(agent.live_trunk: a third trunk pass, re-packed weights per step, no prefetch overlap)")
    a = ap.parse_args()
    assert a.run_dir or not (a.save_every or a.resume), "--save_every / --resume need --run_dir"

    env = _Env()
    sample_obs = {"front": np.zeros((1, H, W, 3), np.uint8), "wrist": np.zeros((1, H, W, 3), np.uint8),
                  "state": np.zeros((1, S), np.float32)}
    shapes = a.critic_dims is not None or a.policy_dims is not None
    if a.hidden == 256 and a.activation == "tanh" and a.weight_decay is None and not shapes:
        agent = make_drq_agent(seed=42, sample_obs=sample_obs, sample_action=np.zeros((A,), np.float32), image_keys=KEYS,
                               encoder_type="resnet-pretrained", batch_size=a.batch_size)
    else:
        # make_drq_agent has no width, activation or optimizer argument (launcher.py:79-116 writes hidden_dims and nn.tanh into
        # the call): other ones go to create_drq as they do in the reference, with the launcher's other hyper-parameters
        opt = {} if a.weight_decay is None else {f"{tx}_optimizer_kwargs": {"weight_decay": a.weight_decay}
                                                 for tx in ("actor", "critic", "temperature")}
        mlp = {"activations": a.activation, "use_layer_norm": True, "hidden_dims": [a.hidden, a.hidden]}
        critic_mlp, policy_mlp = dict(mlp, hidden_dims=a.critic_dims or mlp["hidden_dims"]), dict(mlp, hidden_dims=a.policy_dims or mlp["hidden_dims"])
        agent = DrQAgent.create_drq(
            42, sample_obs, np.zeros((A,), np.float32), encoder_type="resnet-pretrained", use_proprio=True, image_keys=KEYS,
            policy_kwargs={"tanh_squash_distribution": True, "std_parameterization": "exp", "std_min": 1e-5, "std_max": 5},
            critic_network_kwargs=critic_mlp, policy_network_kwargs=policy_mlp, temperature_init=1e-2, discount=0.96,
            backup_entropy=False, critic_ensemble_size=10, critic_subsample_size=2, batch_size=a.batch_size, mlp_shapes=shapes, **opt)
        if shapes:
            print(f"critic hidden_dims {list(agent.core.critic_dims)}, policy hidden_dims {list(agent.core.policy_dims)}", flush=True)
        if a.weight_decay is not None:
            print(f"weight_decay {a.weight_decay:g} in all three optimizers: live trunk {agent.live_trunk}", flush=True)
    replay_buffer = make_replay_buffer(env, capacity=200000, type="memory_efficient_replay_buffer", image_keys=KEYS)
    demo_buffer = make_replay_buffer(env, capacity=10000, type="memory_efficient_replay_buffer", image_keys=KEYS)
    stores, update_steps = {"replay": replay_buffer, "demo": demo_buffer}, 0
    if a.resume:
        update_steps = restore_run(a.run_dir, agent, stores)
        print(f"resumed at {update_steps} grad-steps: replay size {len(replay_buffer)}, demo size {len(demo_buffer)}", flush=True)
    else:
        for tr in itertools.islice(transition_stream(KEYS, H, W, 3, 1, S, A, 100, 99), 2000):   # 20 demo trajectories
            demo_buffer.insert(tr)

    # ---- learner endpoint (async_drq_sim.py:202-212)
    stats_log = []

    def stats_callback(type: str, payload: dict) -> dict:   # noqa: A002
        assert type == "send-stats", f"Invalid request type: {type}"
        stats_log.append(payload)
        return {}

    cfg = make_trainer_config(port_number=a.port, broadcast_port=a.port + 1)
    server = TrainerServer(cfg, request_callback=stats_callback)
    server.register_data_store("actor_env", replay_buffer)
    server.start(threaded=True)

    # ---- mock actor (async_drq_sim.py:91-177 without the env / policy): its own thread, like the actor process
    stop_actor, networks = threading.Event(), []

    def actor_loop():
        data_store = QueuedDataStore(2000)
        client = TrainerClient("actor_env", "localhost", make_trainer_config(a.port, a.port + 1), data_store, wait_for_server=True)
        client.recv_network_callback(lambda params: networks.append(sorted(params.keys())))
        for step, tr in enumerate(transition_stream(KEYS, H, W, 3, 1, S, A, 100, 1234)):
            if stop_actor.is_set():
                break
            data_store.insert(tr)
            if step % a.steps_per_update == 0:
                client.update()
            if step % 200 == 0:
                client.request("send-stats", {"timer": {"total": time.time()}})
            if step >= a.training_starts:
                time.sleep(0.005)                                      # a real actor steps its env at 10-20 Hz
        client.stop()

    actor_thread = threading.Thread(target=actor_loop, name="mock-actor", daemon=True)
    actor_thread.start()
    while len(replay_buffer) < a.training_starts:                      # :215-226 "Filling up replay buffer"
        time.sleep(0.05)
    server.publish_network(agent.state.params)                          # :229 initial network

    half = {"batch_size": a.batch_size // 2, "pack_obs_and_next_obs": True, "lazy": True}
    replay_iterator, demo_iterator = replay_buffer.get_iterator(sample_args=half), demo_buffer.get_iterator(sample_args=half)
    t0, steps_before = time.time(), update_steps
    for step in range(a.steps):
        for _ in range(a.critic_actor_ratio - 1):                        # async_drq_sim.py:266-281
            batch = concat_batches(next(replay_iterator), next(demo_iterator), axis=0)
            agent, critics_info = agent.update_critics(batch)
            update_steps += 1
        batch = concat_batches(next(replay_iterator), next(demo_iterator), axis=0)
        agent, update_info = agent.update_high_utd(batch, utd_ratio=1)   # :283-292
        update_steps += 1
        if step > 0 and step % a.steps_per_update == 0:                  # :295-297
            server.publish_network(agent.snapshot if a.publish == "snapshot" else agent.state.params)
        if step % a.log_period == 0:
            info = update_info.resolve()                                 # synchronises; the reference logs to wandb here
            print(f"step {step:5d} updates {update_steps:6d} critic_loss {info['critic']['critic_loss']:.4f} "
                  f"actor_loss {info['actor']['actor_loss']:.4f} temperature {info['actor']['temperature']:.4f} "
                  f"{(update_steps - steps_before) / (time.time() - t0):.1f} grad-steps/s", flush=True)
        if a.eval_every and step % a.eval_every == 0:
            # "does the critic overestimate on the demonstrations, how likely are their actions?" -- forward_critic /
            # forward_policy(train=False).log_prob in the reference; a stored action at exactly +-1 has no finite log-prob
            ev = agent.evaluate_batch(demo_buffer.sample(min(a.batch_size, 64), pack_obs_and_next_obs=True, lazy=True))
            lp = ev["log_prob"][np.isfinite(ev["log_prob"])]
            print(f"step {step:5d} demo batch: mean Q {ev['q'].mean():.4f} (target copy {ev['q_target'].mean():.4f}) "
                  f"mean log-prob of its actions {lp.mean() if lp.size else float('nan'):.4f} over {lp.size}/{ev['log_prob'].size} "
                  f"rows inside (-1, 1); mean std {ev['std'].mean():.4f}", flush=True)
        if a.checkpoint_path and a.checkpoint_period and step and step % a.checkpoint_period == 0:
            if a.publish == "snapshot":     # the copy leaves the device behind the next updates; the file is written from pinned memory
                with agent.snapshot(("params", "target_params", "opt_states"), slots=1) as snap:
                    save_checkpoint(a.checkpoint_path, snap, step=snap.step, keep=20)
            else:
                save_checkpoint(a.checkpoint_path, agent, step=update_steps, keep=20)   # :303-307
        if a.save_every and step and step % a.save_every == 0:
            save_run(a.run_dir, agent, stores, step=update_steps, keep=2)
    stop_actor.set()
    actor_thread.join(timeout=10)
    time.sleep(0.2)
    server.stop()
    print(f"done: {update_steps} grad-steps; transport: {server.transport}; server stats {server.stats}; "
          f"actor received {len(networks)} networks {networks[-1] if networks else None}; replay size {len(replay_buffer)}", flush=True)
    encode_s = list(server.encode_seconds)
    if encode_s:
        print(f"publisher thread: {len(encode_s)} encodes, median {1e3 * float(np.median(encode_s)):.1f} ms, "
              f"max {1e3 * max(encode_s):.1f} ms each (pickle + LZ4)", flush=True)
    assert server.stats["transitions"] >= a.training_starts and len(networks) >= 1 and stats_log
    if a.publish == "snapshot":     # every snapshot handed over was sent or, when a newer one overtook it, dropped -- none was lost
        handed = sum(1 for step in range(1, a.steps) if step % a.steps_per_update == 0)
        assert server.stats["published"] - 1 + server.stats.get("publish_dropped", 0) == handed, server.stats
        assert "publish_refused_nonfinite" not in server.stats, server.stats


if __name__ == "__main__":
    main()
