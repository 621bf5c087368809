"""The device-resident features taking turns on two side streams (tests/mixed_streams_cases.py): factorize_device on one,
solve_device on the other behind an event, then selinv_device, the gradient through the solve, the gradient through the
factor, schur_device and residual_device, the stream switched at every turn and no host wait in between, twice.  They all
order the engine stream with the plan's one pair of events; no other test crosses features on different streams.  Every
result is held to the reference and the bar of that feature's own side-stream case.

The body runs in a fresh child process, as those of tests/test_gpu_schur.py do: torch has to be imported before the engine
library is loaded."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_features_alternate_between_two_streams():
    p = subprocess.run([sys.executable, os.path.join(HERE, "mixed_streams_cases.py")], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    print(p.stderr[-4000:])
    assert p.returncode == 0 and "CASE OK" in p.stdout, p.returncode
