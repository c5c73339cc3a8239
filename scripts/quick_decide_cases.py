"""The cases of tests/test_gpu_quick_decide.py, run through ndtpso_align_pairs with one build of the library and saved:

    python scripts/quick_decide_cases.py shipped|noquick|quickcount out.npz     # GPU box

shipped: the library as built; noquick: -DNDTPSO_QUICK_DECIDE=0 -DNDTPSO_EARLY_STOP=0, every evaluation through the fp64 lane
reduce; quickcount: -DNDTPSO_COUNT_QUICK, `gbest_updates` holds the evaluations decided quickly.  The two first must agree bit
for bit in everything saved here (the quick decision changes how many items reach the fp64 reduce, not one decision).
Prints one JSON line: per case and score mode the arbitrated comparisons and, for quickcount, the share decided quickly.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("n_points", "cost_evals", "rounds", "status", "arbitrated")
MODES = ("exact", "f32", "f64")


def cases():
    import numpy as np
    from ndtpso_slam_amd import synth
    dev = (0.1, 0.1, 3.1415e-3)
    out = {}
    p = synth.make_pairs(16, seed=2024, total_pairs=512)
    out["beams1081"] = dict(p=p, ref=p.ref_ranges, new=p.new_ranges, guess=(0, 0, 0), dev=dev, I=15, P=20)  # 17 chunks: trips of 6 + 6 + 5
    q = synth.make_pairs(16, n_beams=361, seed=2024, total_pairs=512)
    out["beams361"] = dict(p=q, ref=q.ref_ranges, new=q.new_ranges, guess=(0, 0, 0), dev=dev, I=15, P=20)   # two items per wave
    # 1000 valid beams: everything behind the 1000th valid beam of scan B is a miss -- not a whole number of chunks
    new = p.new_ranges[:8].copy()
    for b in range(new.shape[0]):
        valid = np.flatnonzero(new[b] > 0)
        assert valid.size >= 1000
        new[b, valid[999] + 1:] = 0.0
    out["valid1000"] = dict(p=p, ref=p.ref_ranges[:8], new=new, guess=(0, 0, 0), dev=dev, I=15, P=20, n_points=1000)
    # a converged swarm: scan B is scan A, the guess is the truth, the swarm starts within a micrometre of it -- the costs
    # crowd inside the arbitration margin and just outside it, where the quick decision must decline
    out["converged"] = dict(p=p, ref=p.ref_ranges[:8], new=p.ref_ranges[:8], guess=(0, 0, 0), dev=(1e-6, 1e-6, 1e-8), I=30, P=20)
    return out


def main():
    which, dst = sys.argv[1], sys.argv[2]
    from ndtpso_slam_amd import build as b
    if which != "shipped":
        os.environ["NDTPSO_LIB"] = b.build_variant(which)
    else:
        os.environ.pop("NDTPSO_LIB", None)
    # a handful of pairs would each be spread over a cluster of workgroups, whose evaluation loop is not the one in question:
    # every alignment on one workgroup, as the pairs of a full batch are
    os.environ["NDTPSO_CLUSTER"] = "0"
    import numpy as np
    from ndtpso_slam_amd import capi
    ctx = capi.Context(0)
    mode_of = {"exact": capi.SCORE_EXACT, "f32": capi.SCORE_F32, "f64": capi.SCORE_F64}
    saved, report = {}, {}
    for name, c in cases().items():
        p = c["p"]
        geom = capi.ScanGeom(p.n_beams, float(p.angle_min), float(p.angle_inc), float(p.range_max), 0.1)
        seeds = p.seeds[:c["ref"].shape[0]]
        for m in MODES:
            pose, cost, st = ctx.align_pairs(c["ref"], c["new"], geom, capi.Grid(60, 60, 0.5), c["guess"], c["dev"],
                                             capi.PSOConfig.make(c["I"], c["P"]), seeds=seeds, mode=mode_of[m])
            if "n_points" in c:
                assert (st["n_points"] == c["n_points"]).all(), st["n_points"]
            key = name + "." + m
            saved[key + ".pose"] = pose
            saved[key + ".cost"] = cost
            for f in FIELDS:
                saved[key + "." + f] = st[f]
            report[key] = dict(arbitrated=int(st["arbitrated"].sum()), flagged=int((st["status"] != 0).sum()),
                               cost_evals=int(st["cost_evals"].sum()))
            if which == "quickcount":
                report[key]["decided_quickly"] = int(st["gbest_updates"].sum())
    ctx.close()
    np.savez(dst, **saved)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
