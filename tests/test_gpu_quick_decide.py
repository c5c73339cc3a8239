"""The quick decision (ndtpso_kernels.hpp: wave_sum_f32 / quick_loser) changes how many evaluations reach the fp64
lane reduce and not one decision: the shipped library and the build without it (-DNDTPSO_QUICK_DECIDE=0 -DNDTPSO_EARLY_STOP=0)
return the same bits through ndtpso_align_pairs, in all three score modes.  Each build runs scripts/quick_decide_cases.py once,
in a process of its own (the library is selected per process with NDTPSO_LIB); the tests compare what the two saved."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHAT = ("pose", "cost", "status", "n_points", "cost_evals", "rounds", "arbitrated")
MODES = ("exact", "f32", "f64")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("quick_decide")
    out = {}
    for which in ("shipped", "noquick"):
        dst = str(d / (which + ".npz"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "quick_decide_cases.py"), which, dst], capture_output=True,
                           text=True, timeout=900, env={k: v for k, v in os.environ.items() if k != "NDTPSO_LIB"})
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        report = json.loads(r.stdout.strip().splitlines()[-1])
        print(which, json.dumps(report))
        out[which] = (dict(np.load(dst)), report)
    return out


# beams1081: the one-item loop, 17 chunks in trips of 6 + 6 + 5; beams361: two items per wave; valid1000: a scan whose length
# is no whole number of chunks, the padding masked; converged: costs inside the margin and just outside it
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ("beams1081", "beams361", "valid1000", "converged"))
def test_same_bits_with_and_without_the_quick_decision(runs, case, mode):
    a, b = runs["shipped"][0], runs["noquick"][0]
    for w in WHAT:
        k = "%s.%s.%s" % (case, mode, w)
        if w == "cost_evals":
            continue
        assert a[k].tobytes() == b[k].tobytes(), (k, a[k], b[k])
    # cost_evals counts the evaluations thrown away behind a gbest update as well, and in the kernels that deal a phase's
    # items by ticket how many were in flight then depends on timing (include/ndtpso_hip.h says so: two runs of ONE library
    # differ in it -- the converged case, build without the quick decision: 6533 against 6547 evaluations of 8 alignments in the
    # exact mode, 6529 against 6532 in the fp64 mode -- while poses, costs,
    # rounds and arbitrated comparisons do not).  What is fixed is what a phase establishes -- equal here, since `rounds` and
    # every decision are -- and what can differ is bounded: a wave has at most two items in flight (the two-items-per-wave
    # form) when the phase's first improver turns up, a workgroup at most 16 waves, so 32 evaluations per phase.
    k = "%s.%s." % (case, mode)
    ea, eb = a[k + "cost_evals"].astype(np.int64), b[k + "cost_evals"].astype(np.int64)
    print(k + "cost_evals", ea.tolist(), eb.tolist())
    assert (np.abs(ea - eb) <= 32 * a[k + "rounds"].astype(np.int64)).all(), (ea, eb)


def test_the_converged_case_has_near_ties(runs):
    # (otherwise it tests nothing: the comparisons the quick decision must leave alone are the arbitrated ones)
    for which in ("shipped", "noquick"):
        assert runs[which][1]["converged.exact"]["arbitrated"] > 0, runs[which][1]


def test_exact_mode_is_the_fp64_mode_bit_for_bit(runs):
    a = runs["shipped"][0]
    for w in ("pose", "cost"):
        assert a["beams1081.exact." + w].tobytes() == a["beams1081.f64." + w].tobytes(), w
    assert (a["beams1081.exact.status"] == 0).all()
