"""ppsci.loss.mtl.PCGrad / Relobralo / AGDA (/root/reference/ppsci/loss/mtl/pcgrad.py:27-124, relobralo.py:24-127,
agda.py:27-154): aggregators that act on the per-loss gradients themselves, not through scalar loss weights fixed
before the step.

The reference back-propagates every loss on its own inside the aggregator and rewrites `param.grad`.  On the fused HIP
path the Solver runs one masked forward + reverse pass of the engine per loss key (as it does for GradNorm / NTK), keeps
the K flat gradients as the rows of one persistent [K, P] matrix, and two kernels do the rest on the device
(csrc/grad_surgery.inc): the Gram matrix of the rows with the aggregator's rule in Gram space, and the weighted
combination of the rows with the Adam update behind it.  DESIGN.md 4.14 has the derivation and the measured cost.

Deviations from the reference, on purpose:
  * PCGrad: the reference divides by <g_k, g_k> even when it is 0, which turns every gradient into NaN; here a loss
    whose gradient is exactly zero is skipped as a projection target.
  * PCGrad: the reference's own training loop calls float() on the aggregator object that PCGrad.__call__ returns
    (solver/train.py:145), so the class works on its own but not in that loop; here the logged `loss` is the plain
    sum of the terms.
  * Relobralo: rho is drawn from numpy's global generator (float(np.random.random() < beta)), the reference draws it
    from paddle's (paddle.bernoulli); the two streams cannot be matched, beta = 0 and beta = 1 are deterministic in both.
    The K-element rule is evaluated in float64 (float32 tensors in the reference).
  * Data parallelism: the reference projects BEFORE its gradient all-reduce, so every rank may shuffle on its own.  Here the
    surgery runs behind the all-reduce of the gradient matrix, on every rank, so the ranks must apply ONE order / rho: every
    rank draws (the streams are consumed alike), rank 0's draw travels in spare slots of the all-reduced buffer
    (Solver._share_over_ranks) -- whatever the ranks' numpy states are.
  * AGDA is not built: the reference's _refine_grads reads the local Lf_smooth_kM, which is only bound when
    step % M == 0 (agda.py:113-117), so it raises on every other step and there is no behaviour to reproduce."""
from typing import Dict, List, Optional, Sequence

import numpy as np

from .base import LossAggregator


class PCGrad(LossAggregator):
    """Projecting conflicting gradients (Yu et al. 2020).  For every loss i and every loss k in a freshly shuffled order:
    g_i <- g_i - min(<g_i, g_k> / <g_k, g_k>, 0) g_k with the ORIGINAL g_k; the parameter gradient is sum_i g_i."""

    should_persist = False
    grad_matrix = True     # Solver: K masked passes into a [K, P] matrix, then grad_surgery + grad_combine
    device_rule = True     # the combination weights are computed on the device from the Gram matrix (no host sync)

    def __init__(self, model) -> None:
        super().__init__(model)

    def draw_order(self, keys: Sequence[str]) -> List[int]:
        """One np.random.shuffle of the key list per step (pcgrad.py:64-65); returned as positions in `keys`."""
        shuffled = list(keys)
        np.random.shuffle(shuffled)
        return [list(keys).index(k) for k in shuffled]

    def __call__(self, losses: Dict[str, float], step: int = 0):
        """The logged total: the plain sum of the terms (see the module docstring)."""
        assert len(losses) > 0, f"Number of given losses({len(losses)}) can not be empty."
        self.step = step
        total = 0.0
        for i, key in enumerate(losses):
            total = losses[key] if i == 0 else total + losses[key]
        return total


class Relobralo(LossAggregator):
    """Relative loss balancing with random lookback (Bischof & Kraus 2021): a pure function of the loss values.  The weights
    of step n depend on the losses of step n, so they cannot be applied through the residual scales before the pass (as
    GradNorm's are); the Solver applies them to the per-loss gradient matrix afterwards."""

    should_persist = True
    grad_matrix = True
    device_rule = False    # the rule needs the K loss values on the host (one sync per step; the reference syncs here too)

    def __init__(self, num_losses: int, alpha: float = 0.95, beta: float = 0.99, tau: float = 1.0, eps: float = 1e-8) -> None:
        super().__init__(None)
        self.num_losses, self.alpha, self.beta, self.tau, self.eps = num_losses, alpha, beta, tau, eps
        self.losses_init = np.zeros(num_losses)
        self.losses_prev = np.zeros(num_losses)
        self.lmbda = np.ones(num_losses)

    @staticmethod
    def _softmax(vec: np.ndarray) -> np.ndarray:
        max_item = vec.max()
        return np.exp(vec - max_item) / np.exp(vec - max_item).sum()

    def _compute_bal(self, losses_vec1: np.ndarray, losses_vec2: np.ndarray) -> np.ndarray:
        return self.num_losses * self._softmax(losses_vec1 / (self.tau * losses_vec2 + self.eps))

    def draw_rho(self) -> float:
        """relobralo.py:107, paddle.bernoulli(beta), from numpy's global generator."""
        return float(np.random.random() < self.beta)

    def __call__(self, losses: Dict[str, float], step: int = 0, rho: Optional[float] = None) -> float:
        """relobralo.py:90-127: updates lmbda / losses_init / losses_prev and returns the re-weighted total; `weights()` then
        gives the weights of THIS step's gradient.  `rho`: the step's draw when the caller made it (the Solver under data
        parallelism, where every rank must apply rank 0's); drawn here otherwise."""
        assert len(losses) == self.num_losses, (
            f"Length of given losses({len(losses)}) should be equal to num_losses({self.num_losses}).")
        self.step = step
        losses_stacked = np.asarray([float(v) for v in losses.values()], dtype=np.float64)
        if self.step == 0:
            loss = losses_stacked.sum()
            self.losses_init = losses_stacked.copy()
        else:
            # 1. update lambda_hist
            rho = self.draw_rho() if rho is None else float(rho)
            lmbda_hist = rho * self.lmbda + (1 - rho) * self._compute_bal(losses_stacked, self.losses_init)
            # 2. update lambda
            self.lmbda = self.alpha * lmbda_hist + (1 - self.alpha) * self._compute_bal(losses_stacked, self.losses_prev)
            # 3. compute reweighted total loss with lambda
            loss = (losses_stacked * self.lmbda).sum()
        # update losses_prev at the end of each step
        self.losses_prev = losses_stacked.copy()
        return float(loss)

    def weights(self) -> np.ndarray:
        """The weights the last __call__ gave its losses: ones at step 0 (the plain sum), lmbda afterwards."""
        return np.ones(self.num_losses) if self.step == 0 else self.lmbda

    def state_dict(self):
        return {"losses_init": self.losses_init.copy(), "losses_prev": self.losses_prev.copy(), "lmbda": self.lmbda.copy()}

    def set_state_dict(self, state):
        for k in ("losses_init", "losses_prev", "lmbda"):
            setattr(self, k, np.asarray(state[k], dtype=np.float64).reshape(self.num_losses).copy())


class AGDA(LossAggregator):
    def __init__(self, model=None, M: int = 100, gamma: float = 0.999) -> None:
        raise NotImplementedError(
            "AGDA is not built: the reference's AGDA._refine_grads reads the local Lf_smooth_kM, which is only bound when "
            "step % M == 0 (ppsci/loss/mtl/agda.py:113-117), so it raises on every other step and defines no behaviour "
            "to reproduce")
