"""Worker of tests/test_mtl_distributed.py: one rank of a gloo data-parallel PCGrad / Relobralo run on the CPU SIMT emulator.
argv: output directory, aggregator (pcgrad | relobralo), dp_reduce (sum | mean)."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import ppsci
    from oracle import taylor_np as T
    from paddlescience_amd import device
    from ppsci.autodiff import jacobian
    from tests.common import set_model_weights
    from tests.emu import build_emu

    outdir, kind, dp_reduce = sys.argv[1], sys.argv[2], sys.argv[3]
    build_emu.inject()
    device.set_device("cpu")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        dist.init_process_group("gloo")
    rank = dist.get_rank() if world > 1 else 0
    # the ranks' numpy generators are in DIFFERENT states (nobody has to seed them alike): rank 0's draws are what every rank
    # applies, and rank 0 is seeded like the one-rank run
    np.random.seed(0 if rank == 0 else 12345 + rank)
    model = ppsci.arch.MLP(("x", "y"), ("u",), 2, 16, "tanh")
    set_model_weights(model, T.make_net(2, [16, 16], 1, seed=7, bias_scale=0.05))
    N = 64
    X = np.random.default_rng(3).uniform(0, 1, (N, 2)).astype(np.float32)
    lab = {"laplace": np.zeros((N, 1), np.float32), "u": (np.cos(X[:, :1]) * np.cosh(X[:, 1:])).astype(np.float32),
           "ux": np.full((N, 1), -2.0, np.float32)}
    cfg = {"dataset": {"name": "NamedArrayDataset", "input": {"x": X[:, :1], "y": X[:, 1:]}, "label": lab},
           "batch_size": N // world, "sampler": {"name": "BatchSampler", "shuffle": False, "drop_last": True}}
    exprs = {**ppsci.equation.Laplace(dim=2).equations, "u": lambda out: out["u"], "ux": lambda out: jacobian(out["u"], out["x"])}
    cst = ppsci.constraint.SupervisedConstraint(cfg, ppsci.loss.MSELoss("mean"), exprs, name="EQ")
    opt = ppsci.optimizer.Adam(learning_rate=1e-3)(model)
    agg = ppsci.loss.mtl.PCGrad(model) if kind == "pcgrad" else ppsci.loss.mtl.Relobralo(3, beta=0.5, tau=0.5)
    solver = ppsci.solver.Solver(model, {"EQ": cst}, outdir, opt, epochs=4, iters_per_epoch=1, log_freq=1,
                                 loss_aggregator=agg, dp_reduce=dp_reduce)
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda t, *a, **k: calls.append(t.numel()) or real(t, *a, **k)
    solver.train()
    dist.all_reduce = real
    np.savez(os.path.join(outdir, f"result_w{world}_r{rank}.npz"), params=model.flat_params.numpy(),
             loss=np.asarray(solver.last_losses["loss"]), allreduce=np.asarray(calls, dtype=np.int64),
             G=solver._mtl["G"].numpy(), buf=np.asarray(solver._mtl["buf"].numel()),
             lmbda=np.asarray(getattr(agg, "lmbda", np.zeros(3))))
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
