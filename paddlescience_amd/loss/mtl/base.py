"""ppsci.loss.mtl.LossAggregator (/root/reference/ppsci/loss/mtl/base.py:28-68)."""


class LossAggregator:
    should_persist = False
    per_loss_grad = False  # GradNorm / NTK: the Solver supplies per-key gradient norms at update steps
    grad_matrix = False    # PCGrad / Relobralo: the Solver combines the rows of a per-key gradient matrix every step

    def __init__(self, model=None) -> None:
        self.model = model
        self.step = 0

    def __call__(self, losses, step: int = 0):
        raise NotImplementedError
