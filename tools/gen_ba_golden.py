"""Write the bundle adjustment test vectors, tests/golden/ba_*.npz (CPU only).

Runs the reference's ``bundle_adj.traverse`` for badjust in {none, incr, last} on seeded
synthetic match sets and stores plain arrays: the inputs, the cameras ``traverse`` returns, the
pairs the gate kept, every ``optimize`` call's initial loss, candidate losses and accept
decisions, and the reference's helpers on fixed inputs.  The reference is imported from the
directory given by --reference at generation time; nothing of it is stored but its outputs.
The LM record is taken from the outside: the module's ``residuals`` and ``loss`` are wrapped
while ``optimize`` runs, and a candidate counts as accepted when the adjuster holds its camera
list afterwards.

    python tools/gen_ba_golden.py --reference <dir of the reference>
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pano360_amd.bundle_adj import rotation_to_mat  # noqa: E402
from ba_model import flatten_matches, synthetic_matches  # noqa: E402

MODES = ("none", "incr", "last")
# (name, seed, n_cameras, matches per pair, unreached camera, gated pair)
SETS = (("ring8", 11, 8, 120, 7, (0, 3)),
        ("ring6", 23, 6, 90, None, (1, 4)))


class Recorder:
    """Wraps the reference module's residuals / loss / optimize."""

    def __init__(self, mod):
        self.mod, self.calls, self.active = mod, [], None
        self.orig = (mod.residuals, mod.loss, mod.IncrementalBundleAdjuster.optimize)
        rec = self

        def residuals(cameras, matches):
            if rec.active is not None:
                call = rec.active
                if len(call["cands"]) > 1:      # (the first entry is the initial state)
                    call["accepted"].append(call["iba"].cameras is call["cands"][-1])
                call["cands"].append(cameras)
            return rec.orig[0](cameras, matches)

        def loss(res):
            value = rec.orig[1](res)
            if rec.active is not None:
                rec.active["losses"].append(float(value))
            return value

        def optimize(iba):
            rec.active = {"iba": iba, "cands": [], "losses": [], "accepted": []}
            try:
                rec.orig[2](iba)
                call = rec.active
                if len(call["cands"]) > 1:
                    call["accepted"].append(iba.cameras is call["cands"][-1])
                rec.calls.append(call)
            finally:
                rec.active = None

        mod.residuals, mod.loss = residuals, loss
        mod.IncrementalBundleAdjuster.optimize = optimize

    def restore(self):
        self.mod.residuals, self.mod.loss, self.mod.IncrementalBundleAdjuster.optimize = self.orig


def run_mode(ref, matches, n_cams, mode):
    rec = Recorder(ref)
    kept = []
    orig_init = ref.IncrementalBundleAdjuster.__init__

    def init(self, *args, **kw):
        orig_init(self, *args, **kw)
        kept.append(self)
    ref.IncrementalBundleAdjuster.__init__ = init
    try:
        imgs = [np.full(1, i) for i in range(n_cams)]
        cams = ref.traverse(imgs, matches, badjust=mode)
    finally:
        ref.IncrementalBundleAdjuster.__init__ = orig_init
        rec.restore()
    iba = kept[0]
    out = {"index": np.array([int(c.img[0]) for c in cams]),
           "rot": np.stack([c.rot for c in cams]), "intr": np.stack([c.intr for c in cams]),
           "pairs": np.array([(a, b) for a, b, _ in iba.matches], np.int64).reshape(-1, 2)}
    n_calls = len(rec.calls)
    out["opt_n_cameras"] = np.array([sum(c is not None for c in call["cands"][0])
                                     for call in rec.calls], np.int64)
    out["opt_len"] = np.array([len(call["losses"]) - 1 for call in rec.calls], np.int64)
    out["opt_initial"] = np.array([call["losses"][0] for call in rec.calls])
    out["opt_losses"] = np.array([x for call in rec.calls for x in call["losses"][1:]])
    out["opt_accepted"] = np.array([x for call in rec.calls for x in call["accepted"]], bool)
    assert len(out["opt_losses"]) == len(out["opt_accepted"]), n_calls
    return out, iba, rec.calls


def state_arrays(cameras):
    idx = [i for i, c in enumerate(cameras) if c is not None]
    return (np.array(idx), np.stack([cameras[i].intr for i in idx]),
            np.stack([cameras[i].rot for i in idx]))


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reference", required=True, help="directory of the reference sources")
    parser.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = parser.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    ref = importlib.import_module("bundle_adj")

    for name, seed, n_cams, per_pair, unreached, gated in SETS:
        matches, truth = synthetic_matches(seed, n_cams, per_pair, unreached=unreached,
                                           gated=gated)
        flat = flatten_matches(matches)
        data = {"n_cameras": np.array(n_cams), "true_rot": truth[0], "true_focal": truth[1]}
        data.update({f"in_{k}": v for k, v in flat.items()})
        for mode in MODES:
            out, iba, calls = run_mode(ref, matches, n_cams, mode)
            data.update({f"{mode}_{k}": v for k, v in out.items()})
            if mode == "incr":
                # the normal equations at the last optimize call's final state: J at the
                # accepted cameras, r at the accepted cameras and at the rejected last candidate
                call = calls[-1]
                acc, rej = iba.cameras, call["cands"][-1]
                assert acc is not rej and not call["accepted"][-1]
                jac, jtj = ref._jacobian_symbolic(acc, iba.matches)
                res_acc = ref.residuals(acc, iba.matches)
                res_rej = ref.residuals(rej, iba.matches)
                for tag, cams in (("acc", acc), ("rej", rej)):
                    idx, intr, rot = state_arrays(cams)
                    data[f"sys_{tag}_index"], data[f"sys_{tag}_intr"] = idx, intr
                    data[f"sys_{tag}_rot"] = rot
                data["sys_jtj"] = jtj
                data["sys_jtr_acc"], data["sys_jtr_rej"] = jac.T @ res_acc, jac.T @ res_rej
                data["sys_res_acc"], data["sys_res_rej"] = res_acc, res_rej
        # the helpers on fixed inputs
        rng = np.random.default_rng(seed + 1)
        homs = np.stack([h for _, _, h in flat_iter(flat)][:6])
        data["focal_hom"] = homs
        data["focal_ref"] = np.array([ref.get_focal(h) for h in homs])
        rots = [np.eye(3), rotation_to_mat([1e-9, 0, 0]), rotation_to_mat([0, np.pi - 1e-3, 0]),
                rotation_to_mat(rng.normal(0, 0.5, 3)), rotation_to_mat(rng.normal(0, 1.5, 3))]
        data["angle_rot"] = np.stack(rots)
        data["angle_ref"] = np.stack([ref.mat_to_angle(r) for r in rots])
        data["drdv_ref"] = np.stack([ref.dr_dvi(r) for r in rots])
        sets = [truth[0], np.stack([rotation_to_mat(rng.normal(0, 0.3, 3)) @ r
                                    for r in truth[0]])]
        data["straighten_in"] = np.stack(sets)
        data["straighten_ref"] = np.stack([np.stack(ref.straighten(list(s))) for s in sets])
        path = os.path.join(args.out, f"ba_{name}.npz")
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path), "bytes;",
              {m: int(data[f"{m}_opt_len"].sum()) for m in MODES}, "LM iterations")


def flat_iter(flat):
    for k, (i, j) in enumerate(flat["keys"]):
        yield i, j, flat["homs"][k]


if __name__ == "__main__":
    main()
