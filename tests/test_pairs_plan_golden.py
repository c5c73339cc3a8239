"""The fused-pairs plans -- what pairs_plan / make_plan / pick_waves decide, as ndtpso_align_pairs_describe reports it -- against
tests/golden/pairs_plans.npz.  No device needed.

The file was recorded at the parent commit of the change that gave make_plan / pairs_plan / launch_pairs their named requests
(PlanAsk, PairsBatch, PairsLaunch): a host-side refactor must not move a plan.  A change that means to move one re-records it
with scripts/record_pairs_plans.py and says so."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_pairs_plans", os.path.join(ROOT, "scripts", "record_pairs_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pairs_plans_match_the_recorded_ones():
    rec = _recorder()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "pairs_plans.npz"))
    # 7 beam counts x 4 cell sides x 2 frames x 5 populations x 2 batch sizes x 3 score modes
    assert gold["rows"].shape == (7 * 4 * 2 * 5 * 2 * 3, 9)
    assert tuple(gold["key_names"]) == rec.KEY_NAMES and tuple(gold["fields"]) == rec.FIELDS
    keys, rows = rec.describe_all()
    assert np.array_equal(keys, gold["keys"])          # the same configurations, in the same order
    bad = np.flatnonzero((rows != gold["rows"]).any(axis=1))
    assert bad.size == 0, "\n".join(
        "%s: %s, recorded %s" % (dict(zip(rec.KEY_NAMES, keys[i])), dict(zip(rec.FIELDS, rows[i])), list(gold["rows"][i]))
        for i in bad[:10])
