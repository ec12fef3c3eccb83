"""GPU tier: examples/02_mlp_getting_started.py with --trainer -- the guide's workflow with MLPTrainer.step as the loop
body (Adagrad lr 0.1 inside the step's reduction launch) learns on the synthetic split."""
import importlib.util
import inspect
import math
import os

import pytest

pytestmark = pytest.mark.gpu


def _example():
    spec = importlib.util.spec_from_file_location(
        "mlp_example_trainer", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples",
                                            "02_mlp_getting_started.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_getting_started_example_learns_with_the_trainer():
    mod = _example()
    assert inspect.signature(mod.run).parameters["trainer"].default is False      # the default path stays the guide's
    trace = mod.run(epochs=2, log=lambda msg: None, trainer=True)
    assert len(trace) == 3 and all(math.isfinite(v) for v in trace)
    assert trace[-1] > trace[0], trace
