"""CPU: the oracle of the IRNet update step and the dp_mean pass (tests/irn_sgd_ref.py) against torch.

torch.optim.SGD on the CPU is the reference but not bit-defined: its vector body fuses a + alpha b, and which lanes take the vector
body depends on the alignment of the allocation.  So the float32 restatement's distance to torch is MEASURED here (R32_SGD, printed)
and held to 4 x the recorded figure -- a margin over torch, never over the code under test; the float64 form agrees with
torch.double to 1e-12."""
import numpy as np
import pytest
import torch

from oracle import irn_ref
from tests import irn_grad_ref
from tests import irn_sgd_ref as ref

LR, WD, POWER, MAX_STEP = 0.1, 1e-4, 0.9, 7


class TorchPolyOptimizer(torch.optim.SGD):
    """PolyOptimizer as IRNet writes it: the constructor hands weight_decay to SGD's third positional parameter, `momentum`"""

    def __init__(self, params, lr, weight_decay, max_step, momentum=0.9):
        super().__init__(params, lr, weight_decay)
        self.global_step = 0
        self.max_step = max_step
        self.momentum = momentum
        self._initial_lr = [group["lr"] for group in self.param_groups]

    def step(self, closure=None):
        if self.global_step < self.max_step:
            lr_mult = (1 - self.global_step / self.max_step) ** self.momentum
            for i in range(len(self.param_groups)):
                self.param_groups[i]["lr"] = self._initial_lr[i] * lr_mult
        super().step(closure)
        self.global_step += 1


@pytest.fixture(scope="module")
def sd():
    return irn_ref.make_resnet50_irn_state_dict(seed=3)


def _torch_run(sd, steps, dtype, grads):
    """-> (the parameters after `steps` steps as {name: array}, the lr pairs torch used, the optimiser)"""
    edge, dp = irn_grad_ref.param_names("resnet50")
    params = {n: sd[n].detach().clone().to(dtype).requires_grad_(True) for n in edge + dp}
    opt = TorchPolyOptimizer([{"params": [params[n] for n in edge], "lr": LR, "weight_decay": WD},
                              {"params": [params[n] for n in dp], "lr": 10 * LR, "weight_decay": WD}],
                             lr=LR, weight_decay=WD, max_step=MAX_STEP, momentum=POWER)
    lrs = []
    for k in range(steps):
        g = ref.unflatten(grads[k], sd, "resnet50")
        for n, p in params.items():
            p.grad = torch.from_numpy(g[n]).to(dtype)
        opt.step()
        lrs.append((opt.param_groups[0]["lr"], opt.param_groups[1]["lr"]))
    return {n: p.detach().numpy() for n, p in params.items()}, lrs, opt


def _grads(n, steps):
    rng = np.random.default_rng(41)
    return [rng.standard_normal(n).astype(np.float32) for _ in range(steps)]


@pytest.mark.parametrize("steps", [6, 9])
def test_restatement_against_torch(sd, steps):
    """9 steps at max_step = 7 go past the end of the schedule: the rate freezes at its last value"""
    p0 = ref.flat_params(sd, "resnet50")
    b = ref.boundary(sd, "resnet50")
    names = irn_grad_ref.param_names("resnet50")
    assert ref.layout(sd, "resnet50")[0][len(names[0])][1] == b and ref.layout(sd, "resnet50")[0][len(names[0]) - 1][0] == "fc_edge6.bias"
    grads = _grads(p0.size, steps)
    want, lrs, opt = _torch_run(sd, steps, torch.float32, grads)
    # the quirk, pinned: the SGD momentum is the weight-decay value, the groups keep their own weight decay
    assert all(g["momentum"] == WD and g["weight_decay"] == WD and g["dampening"] == 0 and not g["nesterov"] for g in opt.param_groups)
    assert lrs == [ref.poly_lrs(LR, MAX_STEP, POWER, k) for k in range(steps)]  # equal as doubles
    if steps > MAX_STEP:
        assert lrs[-1] == lrs[MAX_STEP - 1] and lrs[MAX_STEP - 1] != lrs[MAX_STEP - 2]
    p, m = p0, np.zeros_like(p0)
    for k in range(steps):
        p, m = ref.sgd_step32(p, grads[k], m, b, *ref.poly_lrs(LR, MAX_STEP, POWER, k), WD, WD)
    got = ref.unflatten(p, sd, "resnet50")
    flat_want = ref.flat_params(want, "resnet50")
    r = float(np.abs(p.astype(np.float64) - flat_want).max() / max(1.0, np.abs(flat_want).max()))
    differ = float((p != flat_want).mean())
    print("R32_SGD after %d steps: max|d| / max(1, max|p|) = %.3e (recorded %.3e), %.1f %% of the elements differ" % (steps, r, ref.R32_SGD,
                                                                                                             100 * differ))
    assert all(got[n].shape == want[n].shape for n in want)
    assert r <= 4 * ref.R32_SGD
    assert np.abs(p - p0).max() > 0.1  # the steps moved the parameters


def test_float64_form_against_torch_double(sd):
    p0 = ref.flat_params(sd, "resnet50", np.float64)
    b = ref.boundary(sd, "resnet50")
    grads = _grads(p0.size, 9)
    want, _, _ = _torch_run(sd, 9, torch.float64, grads)
    p, m = p0, np.zeros_like(p0)
    for k in range(9):
        p, m = ref.sgd_step64(p, grads[k].astype(np.float64), m, b, *ref.poly_lrs(LR, MAX_STEP, POWER, k), WD, WD)
    d = np.abs(p - ref.flat_params(want, "resnet50", np.float64)).max()
    print("float64 form against torch.double: max|d| = %.3e" % d)
    assert d <= 1e-12


def test_flat_params_round_trip(sd):
    flat = ref.flat_params(sd, "resnet50")
    back = ref.unflatten(flat, sd, "resnet50")
    assert all(np.array_equal(back[n], sd[n].numpy()) for n in back)
    lay, n = ref.layout(sd, "resnet50")
    name, at, shape, conv = next(e for e in lay if e[0] == "fc_dp6.0.weight")
    assert conv and flat[at + 5 * shape[0] + 3] == sd[name][3, 5, 0, 0]  # [Cin][Cout]


def test_mean_oracle_against_torch():
    rng = np.random.default_rng(43)
    batches = [(rng.standard_normal((3, 2, 17, 17)) * 4 + np.array([1.5, -0.25]).reshape(1, 2, 1, 1)).astype(np.float32) for _ in range(3)]
    with torch.no_grad():
        want = torch.mean(torch.stack([torch.mean(torch.from_numpy(b), dim=(0, 2, 3)) for b in batches]), dim=0).numpy()
    got = ref.dp_mean64(batches)
    r = float(np.abs(got - want).max() / max(1.0, np.abs(got).max()))
    print("R32_MEAN: max|d| / max(1, max|mean|) = %.3e (recorded %.3e)" % (r, ref.R32_MEAN))
    assert r <= 4 * ref.R32_MEAN
    shift = np.array([0.5, -1.0], np.float32)
    assert np.abs(ref.dp_mean64(batches, shift) - (got - shift)).max() <= 1e-15
