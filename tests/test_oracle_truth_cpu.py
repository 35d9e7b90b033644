"""CPU: the fp64 ground truth (tests/golden/truth_*.npz, written by ``python -m oracle.make_golden truth``) is what the oracle's fp64 mode
computes today, on the inputs of the fp32 fixture beside it.  The small fixtures, alg_relu_noconf and the ResNet-18 backbone are recomputed
here (a few seconds each); the large ones are checked by the generator only.

Agreement: <= 1e-9 relative (fp64 thread-order noise is ~1e-13).  Intermediates are stored as the fp32 rounding of the truth, so for them
the stored value must be the fp32 rounding of a value within 1e-9 of the recomputation: |stored - ours| <= 2^-24 |ours| + 1e-9 max|ours|."""
import os

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import truth as T
from test_oracle_golden import VOL_CASES, build_vol_case

TOL = 1e-9
SMALL = [t for t in VOL_CASES if t.startswith("small_")]


def _same(key, stored, ours):
    stored, ours = np.asarray(stored), np.asarray(ours, np.float64)
    assert stored.shape == ours.shape, (key, stored.shape, ours.shape)
    scale = max(float(np.abs(ours).max()), 1e-300)
    d = np.abs(stored.astype(np.float64) - ours)
    if stored.dtype == np.float64:
        assert d.max() <= TOL * scale, "%s: max|d|/max|truth| = %.3e" % (key, d.max() / scale)
    else:
        assert stored.dtype == np.float32, key
        assert (d <= 2.0 ** -24 * np.abs(ours) + TOL * scale).all(), "%s: not the fp32 rounding of the recomputed truth" % key


def _compare(t, ours):
    keys = [k for k in t.files if not k.startswith("ref32_err/")]
    assert sorted(keys) == sorted(ours), (sorted(keys), sorted(ours))
    for k in keys:
        if k.endswith("digest") or k == "stride":
            assert np.allclose(t[k], ours[k], rtol=1e-12), k
        else:
            _same(k, t[k], ours[k])


@pytest.mark.parametrize("tag", SMALL)
def test_volumetric_truth_reproduces(golden_dir, tag):
    t = np.load(os.path.join(golden_dir, "truth_%s.npz" % tag))
    g = np.load(os.path.join(golden_dir, "vol_%s.npz" % tag))
    assert int(t["stride"]) == T.STRIDE_FACTOR * int(g["stride"])
    _compare(t, T.vol_truth(tag, int(t["stride"])))


def test_algebraic_truth_reproduces(golden_dir):
    t = np.load(os.path.join(golden_dir, "truth_alg_relu_noconf.npz"))
    _compare(t, T.alg_truth("alg_relu_noconf", np.load(os.path.join(golden_dir, "alg_relu_noconf.npz"))))


def test_backbone_truth_reproduces(golden_dir):
    t = np.load(os.path.join(golden_dir, "truth_nets.npz"))
    ours = T.nets_truth(which=(18,))
    assert sorted(ours) == sorted(k for k in t.files if k.startswith("rn18_"))
    for k, v in ours.items():
        if k.endswith("digest"):
            assert np.allclose(t[k], v, rtol=1e-12), k
        else:
            _same(k, t[k], v)


@pytest.mark.parametrize("name", ["vol_" + c for c in VOL_CASES] + ["alg_c1", "alg_relu_noconf", "nets"])
def test_truth_belongs_to_its_fixture(golden_dir, name):
    """Every truth file was computed on its fp32 fixture's inputs (weights, images, stride), holds the fixture's keys and a measured
    reference error for each of them, and is no larger than the fixture (below 8 kB excepted, as in the generator) nor than 1 MiB.  A volumetric
    truth samples the fixture's strided tensors at every T.STRIDE_FACTOR-th point."""
    fixture = os.path.join(golden_dir, name + ".npz")
    tname = name[4:] if name.startswith("vol_") else name
    path = os.path.join(golden_dir, "truth_%s.npz" % tname)
    t, g = np.load(path), np.load(fixture)
    assert os.path.getsize(path) <= max(os.path.getsize(fixture), 8192) and os.path.getsize(path) < T.MAX_BYTES
    if name == "nets":
        keys = [k for k in g.files if k.startswith("rn") and not k.endswith("digest")]
        for nl, _, _ in T.NETS:
            assert np.allclose(t["rn%d_sd_digest" % nl], g["rn%d_sd_digest" % nl], rtol=1e-12)
    else:
        assert np.allclose(t["sd_digest"], g["sd_digest"], rtol=1e-12)
        if "images_digest" in g.files:
            assert np.allclose(t["images_digest"], g["images_digest"], rtol=1e-12)
        if name.startswith("vol_"):
            assert int(t["stride"]) == T.STRIDE_FACTOR * int(g["stride"])
            cfg, sd, inp, c = build_vol_case(tname)
            assert np.allclose(synth.state_dict_checksum(sd), t["sd_digest"], rtol=1e-12)
            keys = [k for k in ("kp", "feat_sub", "unproj_sub", "logits_sub", "vol_sub", "vol_conf") if k in g.files]
        else:
            keys = ["kp2", "conf", "hm_sub", "kp3"]
            assert "kp3_of_ref2d" in t.files and "ref32_err/kp3_of_ref2d" in t.files
    factor = T.STRIDE_FACTOR if name.startswith("vol_") else 1
    for k in keys:
        assert k in t.files and t[k].shape == (T.coarser(g[k], factor) if k.endswith("_sub") else g[k]).shape, k
        e = float(t["ref32_err/" + k])
        assert np.isfinite(e) and e >= 0.0, (k, e)
    assert all(t[k].dtype == np.float64 for k in T.JOINT_KEYS if k in t.files and k != "kp2")
