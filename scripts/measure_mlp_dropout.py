"""Step time of bench.py's workload with Dropout in the MLPs (networks/mlp.py:27-28): bench.py builds the launcher's agent, which has
no argument for the network kwargs, so DrQAgent.create_drq is wrapped here for the duration and bench.main() runs unchanged.
    python scripts/measure_mlp_dropout.py --critic-dropout 0.01 --ensemble 2 [--policy-dropout 0] [--subsample none|N] [bench.py arguments]
prints bench.py's JSON line (the DroQ shape: critic 0.01, ensemble 2, no subsampling).  Under bench.py's default --noise threefry
the masks are drawn in the LayerNorm rows from the call's keys; with --noise hash from the device hash.  Numbers: profiles/README.md."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--critic-dropout", type=float, default=0.01)
    ap.add_argument("--policy-dropout", type=float, default=0.0)
    ap.add_argument("--ensemble", type=int, default=2)
    ap.add_argument("--subsample", default="none")
    mine, rest = ap.parse_known_args()
    import bench
    from serl_amd.agents.drq import DrQAgent
    orig = DrQAgent.__dict__["create_drq"].__func__

    def create_drq(cls, *a, **k):
        k["critic_network_kwargs"] = {**k["critic_network_kwargs"], "dropout_rate": mine.critic_dropout}
        k["policy_network_kwargs"] = {**k["policy_network_kwargs"], "dropout_rate": mine.policy_dropout}
        k["critic_ensemble_size"] = mine.ensemble
        k["mlp_dropout"] = True
        k["critic_subsample_size"] = None if mine.subsample == "none" else int(mine.subsample)
        agent = orig(cls, *a, **k)
        print(f"# create_drq: ensemble {mine.ensemble}, subsample {mine.subsample}, critic dropout {agent.core.critic_dropout}, "
              f"policy dropout {agent.core.policy_dropout}", file=sys.stderr, flush=True)
        return agent
    DrQAgent.create_drq = classmethod(create_drq)
    sys.argv = [os.path.join(ROOT, "bench.py")] + rest
    bench.main()


if __name__ == "__main__":
    main()
