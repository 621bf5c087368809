"""The device-resident features on a seeded random corpus (tests/device_fuzz_corpus.py: Poisson, banded and general random
SPD patterns under natural, nested-dissection and random orderings, block arrows with engineered front shapes, complex
Hermitian and unsymmetric A A' cases, complex Hermitian block arrows on the edges of the complex kernels; n <= 700), the
Schur complement and the condensed solves among them, every result against a dense float64 reference at the bar the project
already holds that feature to.  tests/test_device_fuzz_corpus.py shows on the CPU that the corpus reaches every dispatch
class of the two backward sweeps and of the device solves, every path of the Schur tile kernel's walk and every twin-space
front class of the complex kernels, that the bar stays at 1e-12 and that the references alone use
less than a tenth of it.

One child process per seed (tests/device_fuzz_runner.py: torch has to be imported before the engine library is loaded)
runs all 46 cases; its result is cached, and every feature has its own verdict: the child exited 0, the feature ran at
least one check, none failed.  The worst err / tol of the feature is printed.

Wall time of one child on an MI355X, measured: 14 s for seed 3 and 13 s for seed 11 (46 cases each), most of it the dense
references on the host."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = [3, 11]             # device_fuzz_corpus.SEEDS, NCASE (kept literal here so that collection needs no scipy work)
NCASE = 46
FEATURES = ["factor", "solve", "residual_refine", "selinv", "logdet", "values_grad", "factor_grad", "outer_grad",
            "factorize_device", "budget_bits", "complex_solve", "aat", "schur", "schur_condensed", "complex_arrow"]

_runs = {}


def _run(seed):
    """one child process per seed runs every case; every feature has its own verdict"""
    if seed not in _runs:
        t0 = time.time()
        _runs[seed] = dict(returncode="the child did not finish", result={}, fails=[])    # (it runs once, whatever happens)
        p = subprocess.run([sys.executable, os.path.join(HERE, "device_fuzz_runner.py"), str(seed), str(NCASE)],
                           capture_output=True, text=True, timeout=600)
        print(p.stdout[-20000:])
        print(p.stderr[-4000:])
        print(f"seed {seed}: {time.time() - t0:.1f} s")
        res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        _runs[seed] = dict(returncode=p.returncode, result=json.loads(res[-1]) if res else {},
                           fails=[ln for ln in p.stdout.splitlines() if ln.startswith("FAIL ")])
    return _runs[seed]


def test_the_seeds_are_the_corpus_tests():
    import device_fuzz_corpus as DC
    assert tuple(SEEDS) == DC.SEEDS and NCASE == DC.NCASE


@pytest.mark.parametrize("feature", FEATURES)
@pytest.mark.parametrize("seed", SEEDS)
def test_device_fuzz(seed, feature):
    run = _run(seed)
    assert run["returncode"] == 0, run["returncode"]
    assert feature in run["result"], sorted(run["result"])
    checks, failures, worst = run["result"][feature]
    print(f"seed {seed} {feature}: {checks} checks, {failures} failures, worst err / tol = {worst:.3e}")
    assert checks > 0
    assert failures == 0, [ln for ln in run["fails"] if f" feature {feature} " in ln]
    assert worst <= 1.0
