"""The algebra of the block form of the Gram-Schmidt step — up to four Lanczos iterations per sweep over a basis of raw vectors
that is never rewritten (gs_block.hip, LoopState::enqueue_block) — in numpy, at a size the CPU suite runs in
seconds.  tools/block_gs_model.py is the executable specification the device kernels were written from (same launches, same
formulas, real and complex); the GPU kernels themselves are checked against the oracle in tests/test_gpu_block.py."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("block_gs_model", os.path.join(ROOT, "tools", "block_gs_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_block_form_reproduces_the_recurrence_of_full_reorthogonalisation(model, complex_, m):
    r = model.measure(complex_, m, n=1500, K=120)
    assert r["iterations"] == 120 and r["gate_trips"] == 0
    assert r["dalpha"] <= 1e-12 and r["dbeta"] <= 1e-12
    assert r["orth"] <= 1e-14                          # the basis the record defines
    assert r["maxcoef"] <= 1e-12                       # every coefficient of a raw vector stays eps-sized
    assert abs(r["ritz"]) <= 1e-14                     # the Ritz vector through transformed coefficients
    assert r["orth_flushed"] <= 1e-14 and r["dvec_flushed"] <= 1e-11   # the flush completes the raw vectors in place


def test_both_seeds_must_be_compensated(model):
    """With only the last vector of a block compensated the stored-basis components of the other operand of the next three-term
    update survive and are amplified from block to block."""
    r = model.measure(False, 4, n=1500, K=100, both_seeds=False, gate=np.inf)
    assert r["maxcoef"] >= 1e-8


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_entry_from_the_pair_state_and_an_odd_last_iteration(model, complex_):
    r = model.pair_entry(complex_, n=1200, K=61, at=21)
    assert r["iterations"] == 61 and r["dalpha"] <= 1e-12 and r["dbeta"] <= 1e-12 and r["orth_flushed"] <= 1e-14


@pytest.mark.parametrize("stop", [41, 42, 43, 44])
def test_a_stop_inside_a_block_reads_nothing_behind_it(model, stop):
    r = model.stop_in_block(stop % 2 == 0, stop, n=1200)
    assert r["dropped"] == (2 - stop) % 4
    assert r["dlambda"] <= 1e-12 and abs(r["ritz"]) <= 1e-14 and r["dnorm"] <= 1e-14


@pytest.mark.parametrize("size,pos,trips", [(1e-9, 3, 0), (1e-6, 0, 1), (1e-6, 3, 1), (1e-3, 2, 1)])
def test_planted_components_and_the_gate(model, size, pos, trips):
    """Below the gate planted components are measured and leave no trace; above it the vector stands, the rest of its block is
    dropped, the basis is flushed and single iterations finish the pass — within the recurrence's tolerance either way."""
    r = model.measure(False, 4, n=1500, K=120, plant=(size, 23, pos))
    assert r["gate_trips"] == trips and 0.5 * size <= r["maxcoef"] <= 5 * size
    assert r["dalpha"] <= 1e-12 and r["dbeta"] <= 1e-12 and r["orth_flushed"] <= 1e-14
