"""GPU: bench.py's training step starts over from the seeded initial state after step.reset(), so a run computes the
same step whatever --steps / --warmup came before it, and --dump-outputs writes the same arrays up to rounding."""
import importlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def test_step_after_reset_repeats_the_step_from_the_initial_state(ops):
    bench = importlib.import_module("bench")
    model, step = bench.build_step("cfg2", torch.device("cuda", 0))
    params = list(model.parameters())
    step()                                              # first sight of every shape (pools, plans)

    def from_initial_state():
        step.reset()
        loss, gn = step()
        return (loss.detach().clone(), float(gn), step.last["ctc_output"].detach().clone(),
                [p.detach().clone() for p in params])

    loss_a, gn_a, out_a, w_a = from_initial_state()
    step()
    step()                                              # steps that go on from the weights before them ...
    moved = max(float((p - a).abs().max()) for p, a in zip(params, w_a))
    loss_b, gn_b, out_b, w_b = from_initial_state()     # ... and a step after reset that does not
    ops.check_errors()
    assert moved > 1e-4
    assert torch.equal(loss_a, loss_b) and torch.equal(out_a, out_b)
    assert abs(gn_a - gn_b) <= 1e-5 * abs(gn_a)
    for a, b in zip(w_a, w_b):                          # updates from gradients summed in another order
        assert torch.allclose(a, b, rtol=0, atol=1e-6)
