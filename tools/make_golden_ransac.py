"""Generates tests/golden/ransac_ops.npz, tests/golden/ransac_net.npz and tests/golden/ransac_branches.npz by running the REFERENCE's
RANSACTriangulationNet (CPU, numpy + scipy) where the reference tree is available (the same loader as oracle/make_golden.py).  Writes
only these files, or with --only ops|net|branches only that one (the others stay byte-identical):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_ransac.py [--only branches]

Every problem is solved by the reference twice:
  * "replay": random.seed fixed, random.sample wrapped so that the draws the reference makes are logged (the GPU kernel replays them);
  * "exh":    random.sample patched to yield every pair in lexicographic order with n_iters = C(NV, 2) -- the reference's own code in
              the mode lt_triangulate_ransac runs by default.
For each run the fixture keeps the inlier mask, the point before and after the Huber refinement, scipy's final cost and a
``well_posed`` flag (scipy restarted from the DLT point moved by 1 mm, and scipy with tolerances of 1e-14, land within 1e-5 relative
of the same point).  ransac_branches.npz: NV = 16 and 32 (inlier sets far wider than the 8 views of ransac_ops.npz: the refinement's
per-view starts and 32-bit masks), the exhaustive run only, for tests/test_gpu_ransac_kernels.py.
"""
import itertools
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import ref_loader, spec, synth  # noqa: E402
from ransac_ref import synth_problems  # noqa: E402  (the generator the tests share)

GOLD = os.path.join(ROOT, "tests", "golden")
EPS = 15


class RefRansac:
    """The reference's triangulate_ransac with its random draws, scipy results and the errors it compared with eps observed."""

    def __init__(self, mvn):
        self.mod = sys.modules[mvn.models.triangulation.__name__]
        self.fn = self.mod.RANSACTriangulationNet.triangulate_ransac
        self.mv = mvn.utils.multiview
        self.draws, self.errs, self.costs = [], [], []
        self._sample = random.sample
        self._lsq = self.mod.least_squares
        self._rep = self.mv.calc_reprojection_error_matrix
        self.schedule = None

    def __enter__(self):
        def sample(population, k):
            if self.schedule is not None:
                s = list(next(self.schedule))
            else:
                s = self._sample(sorted(population), k)     # what sample(set) draws for a set of small ints (its iteration order)
            self.draws.append(sorted(s))
            return s

        def lsq(*a, **kw):
            res = self._lsq(*a, **kw)
            self.costs.append(float(res.cost))
            return res

        def rep(*a, **kw):
            m = self._rep(*a, **kw)
            self.errs.append(np.asarray(m).ravel())
            return m
        self.mod.random.sample = sample
        self.mod.least_squares = lsq
        self.mv.calc_reprojection_error_matrix = rep
        return self

    def __exit__(self, *exc):
        self.mod.random.sample = self._sample
        self.mod.least_squares = self._lsq
        self.mv.calc_reprojection_error_matrix = self._rep

    def solve(self, P, pts, direct, schedule=None, n_iters=10):
        """-> (point, inlier list, draws, scipy cost or nan, errors compared with eps)."""
        self.draws, self.errs, self.costs = [], [], []
        self.schedule = iter(schedule) if schedule is not None else None
        X, inl = self.fn(None, P, pts, n_iters=n_iters, reprojection_error_epsilon=EPS, direct_optimization=direct)
        self.schedule = None
        return np.asarray(X, dtype=np.float64), list(inl), list(self.draws), (self.costs[-1] if self.costs else np.nan), list(self.errs)


def huber_solve(mv, P, pts, inl, x0, tight=False):
    from scipy.optimize import least_squares
    Pi, pi = P[inl], pts[inl]
    tol = {"ftol": 1e-14, "xtol": 1e-14, "gtol": 1e-14, "max_nfev": 10000} if tight else {}
    res = least_squares(lambda x: mv.calc_reprojection_error_matrix(np.array([x]), pi, Pi)[0], x0, loss="huber", method="trf", **tol)
    return res.x


def eps_margin(errs):
    """min |error - eps| over the errors the hypothesis loop compared with eps (NaN errors compare false on both sides)."""
    e = np.concatenate(errs)
    e = e[np.isfinite(e)]
    return float(np.abs(e - EPS).min()) if e.size else np.inf


def solve_problem(ref, P, pts, pairs=None, modes=("replay", "exh")):
    """Both runs of one problem (P (NV,3,4) fp32, pts (NV,2) int64).  pairs: replay these draws instead of random ones."""
    NV = len(pts)
    out = {}
    margins = []
    for mode in modes:
        if mode == "replay":
            sched, n = (pairs, len(pairs)) if pairs is not None else (None, 10)
        else:
            sched = list(itertools.combinations(range(NV), 2))
            n = len(sched)
        post, inl, draws, cost, errs = ref.solve(P, pts, True, sched, n)
        pre, inl0, draws0, _, errs0 = ref.solve(P, pts, False, draws, n)
        assert inl0 == inl and draws0 == draws, (inl0, inl, draws0, draws)
        margins.append(eps_margin(errs[:n]))             # the hypothesis-loop comparisons
        dlt = ref.mv.triangulate_point_from_multiple_views_linear(P[inl], pts[inl])
        d = np.random.RandomState(len(margins)).randn(3)
        x1 = huber_solve(ref.mv, P, pts, np.array(inl), dlt + d / np.linalg.norm(d))
        x2 = huber_solve(ref.mv, P, pts, np.array(inl), dlt, tight=True)
        # well posed: scipy restarted 1 mm away lands on the same point, and so does scipy from the DLT point with tolerances of 1e-14
        # (the default ftol = xtol = 1e-8 stop early along the flat valleys of Huber's linear regime)
        well = bool(max(np.abs(x1 - post).max(), np.abs(x2 - post).max()) <= 1e-5 * np.abs(post).max())
        mask = np.zeros(NV, np.uint8)
        mask[inl] = 1
        out[mode] = {"post": post, "pre": pre, "inl": mask, "draws": np.array(draws, np.int32), "cost": cost, "well": well}
    return out, min(margins)


def gen_ops(mvn):
    ref = RefRansac(mvn)
    B, J = 4, 17
    out = {}
    with ref:
        for NV in (2, 3, 4, 8):
            for direct in (0, 1):
                seed = 100 * NV + direct
                while True:
                    rs = np.random.RandomState(seed)
                    random.seed(seed)
                    P, pts = synth_problems(rs, B, NV, J)
                    res = {m: {k: [] for k in ("post", "pre", "inl", "draws", "cost", "well")} for m in ("replay", "exh")}
                    margin = np.inf
                    for b in range(B):
                        for j in range(J):
                            if direct:
                                r, mg = solve_problem(ref, P[b], pts[b, :, j])
                            else:
                                r, mg = solve_problem_nodirect(ref, P[b], pts[b, :, j])
                            margin = min(margin, mg)
                            for m in r:
                                for k in r[m]:
                                    res[m][k].append(r[m][k])
                    if margin >= 1e-6:
                        break
                    print("  NV=%d direct=%d seed %d: an error within %.1e of eps, re-seeding" % (NV, direct, seed, margin))
                    seed += 1000
                tag = "nv%d_d%d" % (NV, direct)
                out[tag + "_P"] = P
                out[tag + "_pts"] = pts
                for m in res:
                    for k, v in res[m].items():
                        a = np.array(v)
                        out["%s_%s_%s" % (tag, m, k)] = a.reshape((B, J) + a.shape[1:])
                nw = int(out[tag + "_replay_well"].sum())
                print("ransac_ops %s: %d problems, %d well posed, min |err - eps| %.2e" % (tag, B * J, nw, margin))
        # the numpy helpers on the NV = 4 problems
        P, pts = out["nv4_d1_P"], out["nv4_d1_pts"]
        lin = np.stack([mvn.utils.multiview.triangulate_point_from_multiple_views_linear(P[b], pts[b, :, j]) for b in range(B) for j in range(J)])
        out["lin_X"] = lin.reshape(B, J, 3)
        X3 = lin.reshape(B, J, 3)[0]
        out["rep_X"] = X3
        out["rep_err"] = np.stack([ref._rep(X3, pts[0, :, j], P[0]) for j in range(J)])      # (J, J 3D points, NV)
    np.savez_compressed(os.path.join(GOLD, "ransac_ops.npz"), **out)


def gen_branches(mvn):
    """B = 1, J = 12 at NV = 16 and 32 from RandomState(NV), direct optimisation, the exhaustive schedule only: solve_problem's record of
    the reference's triangulate_ransac + scipy under the tags nv16_d1 and nv32_d1."""
    ref = RefRansac(mvn)
    B, J = 1, 12
    out = {}
    with ref:
        for NV in (16, 32):
            random.seed(NV)
            P, pts = synth_problems(np.random.RandomState(NV), B, NV, J)
            res = {k: [] for k in ("post", "pre", "inl", "cost", "well")}
            margin = np.inf
            for j in range(J):
                r, mg = solve_problem(ref, P[0], pts[0, :, j], modes=("exh",))
                margin = min(margin, mg)
                for k in res:
                    res[k].append(r["exh"][k])
            assert margin >= 1e-6, (NV, margin)
            tag = "nv%d_d1" % NV
            out[tag + "_P"] = P
            out[tag + "_pts"] = pts
            for k, v in res.items():
                a = np.array(v)
                out["%s_exh_%s" % (tag, k)] = a.reshape((B, J) + a.shape[1:])
            print("ransac_branches %s: %d problems, %d well posed, min |err - eps| %.2e" % (tag, B * J, int(out[tag + "_exh_well"].sum()), margin))
    np.savez_compressed(os.path.join(GOLD, "ransac_branches.npz"), **out)


def solve_problem_nodirect(ref, P, pts):
    """direct_optimization off: the reference returns the DLT point of the inliers; pre == post, no scipy cost."""
    NV = len(pts)
    out, margins = {}, []
    for mode in ("replay", "exh"):
        sched = None if mode == "replay" else list(itertools.combinations(range(NV), 2))
        n = 10 if mode == "replay" else len(sched)
        X, inl, draws, _, errs = ref.solve(P, pts, False, sched, n)
        margins.append(eps_margin(errs[:n]))
        mask = np.zeros(NV, np.uint8)
        mask[inl] = 1
        out[mode] = {"post": X, "pre": X, "inl": mask, "draws": np.array(draws, np.int32), "cost": np.nan, "well": True}
    return out, min(margins)


def gen_net(mvn):
    """The reference RANSACTriangulationNet from experiments/human36m/eval/human36m_ransac.yaml with the backbone shrunk to ResNet-18,
    2 x 4 views of 128^2, synthetic weights."""
    with open(os.path.join(GOLD, "experiments_human36m.json")) as f:
        y = json.load(f)["eval/human36m_ransac.yaml"]
    cfg = synth.AttrDict({"model": y["model"]})
    cfg.model.backbone.update({"name": "resnet18", "num_layers": 18, "init_weights": False, "checkpoint": ""})
    sp = spec.alg_net_spec(18, 17, False)
    sd = synth.make_state_dict(sp, seed=61, basic_block=True)
    inp = synth.make_inputs(2, 4, 128, seed=13)
    net = mvn.models.triangulation.RANSACTriangulationNet(cfg, device="cpu")
    assert list(net.state_dict().keys()) == list(sp.keys())
    net.load_state_dict(sd, strict=True)
    net.eval()
    P = torch.from_numpy(inp["K"] @ np.concatenate([inp["R"], inp["t"]], -1)).float()[None].repeat(2, 1, 1, 1)
    ref = RefRansac(mvn)
    random.seed(2024)
    with ref, torch.no_grad():
        ref.draws = []
        kp3, kp2, hm, conf = net(inp["images"], P, {})
        draws = np.array(ref.draws, np.int32).reshape(2, 17, 10, 2)
        B, NV, J = kp2.shape[:3]
        # per problem: the replayed run's pre / post points, inliers, cost, well_posed (the exhaustive mode on the same inputs too)
        res = {m: {k: [] for k in ("post", "pre", "inl", "cost", "well")} for m in ("replay", "exh")}
        margins = []         # min |error - eps| over the hypothesis comparisons: at random init the views disagree, some may sit on eps
        for b in range(B):
            for j in range(J):
                r, mg = solve_problem(ref, P[b].numpy(), kp2[b, :, j].numpy(), pairs=[tuple(d) for d in draws[b, j]])
                assert np.array_equal(r["replay"]["post"].astype(np.float32), kp3[b, j].numpy())
                margins.append(mg)
                for m in r:
                    for k in res[m]:
                        res[m][k].append(r[m][k])
    top2 = torch.topk(hm.reshape(B, NV, J, -1), 2, dim=-1).values
    out = {"kp3": kp3.numpy(), "kp2": kp2.numpy(), "conf": conf.numpy(), "pairs": draws, "P": P.numpy(),
           "hm_sub": hm.reshape(B * NV, J, 32, 32)[:, :, ::2, ::2].contiguous().numpy(), "hm_absmax": np.float32(hm.abs().max()),
           "margin": (top2[..., 0] - top2[..., 1]).numpy(), "eps_margin": np.array(margins).reshape(B, J),
           "sd_keys": np.array(list(net.state_dict().keys())),
           "sd_shapes": np.array(json.dumps([list(v.shape) for v in net.state_dict().values()])),
           "sd_digest": np.array(synth.state_dict_checksum(sd))}
    for m in res:
        for k, v in res[m].items():
            a = np.array(v)
            out["%s_%s" % (m, k)] = a.reshape((B, J) + a.shape[1:])
    print("ransac_net: kp2 %s %s, %d / %d well posed, min margin %.3e of max|hm| %.3e" % (
        tuple(kp2.shape), kp2.dtype, int(out["replay_well"].sum()), B * J, float(out["margin"].min()), float(out["hm_absmax"])))
    np.savez_compressed(os.path.join(GOLD, "ransac_net.npz"), **out)


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", choices=("ops", "net", "branches"), help="write this fixture alone")
    only = ap.parse_args().only
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mvn = ref_loader.load()
    for name, gen in (("ops", gen_ops), ("net", gen_net), ("branches", gen_branches)):
        if only in (None, name):
            gen(mvn)


if __name__ == "__main__":
    main()
