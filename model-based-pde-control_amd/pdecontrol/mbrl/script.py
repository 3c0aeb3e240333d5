"""Command line of the model-based controller (reference ``pdecontrol/mbrl/script.py``): the reference's flags under
their names and defaults, plus ``--env_config`` (a JSON dict for the env factories).  Builds the config and the
controller, calls ``learn()`` and writes the run's log rows as JSON lines to ``<run dir>/history.jsonl``.

    python -m pdecontrol.mbrl.script --factory KSAutoRegConvolutionalLSTM --cuda --name run0 \\
        --training '{"tau": 5, "initial": {"patience": 5, "batch_size": 128}, "iterations": {"patience": 2, "batch_size": 128}}' \\
        --trainer '{"initial": {"max_steps": 2000}, "iterations": {"max_steps": 200}}' \\
        --curriculum '{"scheduler": "ConstantLengthScheduler", "length": 10}' \\
        --rollout_length_schedule '{"scheduler": "ConstantLengthScheduler", "length": 5}'

``--project`` and ``--offline`` are accepted and unused: there is no wandb here.
"""
import argparse
import json
import os
import sys
import traceback
from argparse import Namespace

import numpy as np
import torch


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    # ---------------- Logging & Evaluation ---------------- #
    parser.add_argument("--project", type=str)
    parser.add_argument("--name", type=str)
    parser.add_argument("--offline", action="store_true")
    parser.add_argument("--agent_eval_freq", type=int, default=50)
    parser.add_argument("--num_eval_episodes", type=int, default=10)
    parser.add_argument("--status_report_freq", type=int, default=5)
    parser.add_argument("--logging_freq", type=int, default=10)
    # ---------------- General Information ---------------- #
    parser.add_argument("--total_timesteps", type=int, default=1000000)
    parser.add_argument("--cuda", action="store_true")
    parser.add_argument("--seed", type=int, default=0)
    # ---------------- Simulation Environment & Rollouts ---------------- #
    parser.add_argument("--env_id", default="KuramotoSivashinskyEnv-v0")
    parser.add_argument("--env_config", type=str, default="{}")
    parser.add_argument("--cpus", type=int, default=10)
    parser.add_argument("--gamma", type=float, default=0.99)
    parser.add_argument("--capacity", type=int, default=1000000)
    parser.add_argument("--rollout_length", type=int, default=1)
    # ---------------- Model-Based Policy Optimization ---------------- #
    parser.add_argument("--learning_starts", type=int, default=20000)
    parser.add_argument("--policy_train_steps_per_sample", type=int, default=5)
    parser.add_argument("--model_buffer_store_iterations", type=int, default=30)
    parser.add_argument("--model_rollouts_per_sample", type=int, default=100)
    parser.add_argument("--model_rollouts_batch_size", type=int, default=100)
    parser.add_argument("--model_buffer_max_capacity", type=int, default=1000000)
    parser.add_argument("--val_split_ratio", type=float, default=0.1)
    parser.add_argument("--rollout_length_schedule", type=str, default="{}")
    # ---------------- Surrogate World Model Training ---------------- #
    parser.add_argument("--surrogate_train_freq", type=int, default=500)
    parser.add_argument("--loss", type=str, default="MSELoss")
    parser.add_argument("--factory", type=str)
    parser.add_argument("--factory_module", type=str)
    parser.add_argument("--model", type=str, default="{}")
    parser.add_argument("--surrogate", type=str, default="{}")
    parser.add_argument("--training", type=str, default="{}")
    parser.add_argument("--curriculum", type=str, default="{}")
    parser.add_argument("--trainer", type=str, default="{}")
    # ---------------- Ensemble of Surrogates ---------------- #
    parser.add_argument("--num_dynamics_models", type=int, default=3)
    parser.add_argument("--num_elite_models", type=int, default=3)
    # ---------------- Soft-Actor Critic ---------------- #
    parser.add_argument("--policy", type=str, default="Gaussian")
    parser.add_argument("--policy_batch_size", default=256, type=int)
    parser.add_argument("--tau", type=float, default=0.005)
    parser.add_argument("--target_entropy", type=float, default=-3.0)
    parser.add_argument("--lr", type=float, default=3e-4)
    parser.add_argument("--alpha", type=float, default=0.2)
    parser.add_argument("--target_update_interval", type=int, default=1)
    parser.add_argument("--hidden_size", type=int, default=256)
    parser.add_argument("--automatic_entropy_tuning", type=bool, default=False)
    return parser


def build_config(args, factory):
    """The reference's config namespace: the factory's defaults overridden by the JSON flags."""
    sections = {name: json.loads(getattr(args, name)) for name in ("model", "surrogate", "training", "curriculum", "trainer")}
    config = {name: {**getattr(factory.defaults, name), **value} for name, value in sections.items()}
    return Namespace(factory=args.factory, loss=args.loss, **config)


def main(argv=None):
    from pdecontrol import architectures
    from pdecontrol.mbrl.mbrl import PDEModelBasedController, RunLog
    args = build_parser().parse_args(argv)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    factory = getattr(architectures, args.factory)()
    config = build_config(args, factory)
    log = RunLog(args.name or "pdecontrol-run")
    mbpo = PDEModelBasedController(args.env_id, factory, config, args, log=log, env_config=json.loads(args.env_config))
    status = 0
    try:
        mbpo.learn()
    except Exception:
        traceback.print_exc(file=sys.stderr)
        status = 1
    finally:
        with open(os.path.join(log.dir, "history.jsonl"), "w") as out:
            for row in log.history:
                out.write(json.dumps(row, default=float) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
