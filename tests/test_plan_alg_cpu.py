"""CPU: the plan-level C ABI of the algebraic and RANSAC models (lt_plan_create_alg / lt_plan_forward_alg) and the algebraic tail kernel
(lt_alg_tail_fwd) are exported, and every configuration error is refused before any device call, with a message that names the field."""
import ctypes as C

import pytest

import lt_hip as H

ERR_INVALID = -1          # LT_ERR_INVALID


def _cfg(**kw):
    c = H.AlgPlanConfig()
    c.model, c.dtype, c.num_layers, c.style_caffe, c.num_joints = H.LT_MODEL_ALG, H.LT_F32, 18, 0, 17
    c.B, c.NV, c.H, c.W = 2, 4, 256, 256
    c.use_confidences, c.heatmap_softmax, c.heatmap_multiplier = 1, 1, 100.0
    c.direct_optimization, c.reprojection_error_epsilon, c.use_graph = 1, 15.0, 1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _weights(names=("backbone.conv1.weight",)):
    arr = (H.NamedTensor * len(names))()
    keep = (C.c_float * 1)()
    for i, n in enumerate(names):
        arr[i].name, arr[i].data, arr[i].ndim, arr[i].shape[0] = n.encode(), C.cast(keep, C.c_void_p), 1, 1
    return arr, keep


def _create(cfg, names=("backbone.conv1.weight",)):
    arr, keep = _weights(names)
    plan = C.c_void_p()
    rc = H.lib().lt_plan_create_alg(C.byref(cfg), arr, len(names), C.byref(plan))
    assert not plan.value
    return rc, H.lib().lt_last_error().decode()


def test_alg_plan_symbols_are_exported():
    lib = C.CDLL(H.LIB_PATH)
    for name in ("lt_plan_create_alg", "lt_plan_forward_alg", "lt_alg_tail_fwd"):
        assert hasattr(lib, name), name
        assert name in H.SIGNATURES, name
    assert H.lib().lt_abi_version() == 1
    assert (H.LT_MODEL_ALG, H.LT_MODEL_RANSAC) == (1, 2)


def test_alg_plan_null_arguments():
    lib = H.lib()
    arr, keep = _weights()
    plan = C.c_void_p()
    cfg = _cfg()
    assert lib.lt_plan_create_alg(None, arr, 1, C.byref(plan)) == ERR_INVALID and "null" in lib.lt_last_error().decode()
    assert lib.lt_plan_create_alg(C.byref(cfg), None, 1, C.byref(plan)) == ERR_INVALID and "null" in lib.lt_last_error().decode()
    assert lib.lt_plan_create_alg(C.byref(cfg), arr, 0, C.byref(plan)) == ERR_INVALID
    assert lib.lt_plan_create_alg(C.byref(cfg), arr, 1, None) == ERR_INVALID
    assert lib.lt_plan_forward_alg(None, 1, 1, 1, None, None, None, None) == ERR_INVALID and "null" in lib.lt_last_error().decode()


@pytest.mark.parametrize("field,value,needle", [
    ("model", 0, "model 0"), ("model", 3, "model 3"),
    ("dtype", H.LT_FP8, "dtype 2"), ("dtype", 7, "dtype 7"),
    ("B", 0, "B 0"), ("NV", 1, "NV 1"), ("H", 16, "H 16"), ("W", 0, "W 0"), ("num_joints", 0, "num_joints 0"),
])
def test_alg_plan_config_validation(field, value, needle):
    for model in (H.LT_MODEL_ALG, H.LT_MODEL_RANSAC):
        cfg = _cfg(model=model)
        setattr(cfg, field, value)
        rc, msg = _create(cfg)
        assert rc == ERR_INVALID and needle in msg and "lt_plan_create_alg" in msg, (model, rc, msg)


@pytest.mark.parametrize("field,value,needle", [("num_joints", 33, "num_joints 33"), ("NV", 33, "NV 33"), ("NV", 1, "NV 1")])
def test_ransac_plan_limits(field, value, needle):
    cfg = _cfg(model=H.LT_MODEL_RANSAC)
    setattr(cfg, field, value)
    rc, msg = _create(cfg)
    assert rc == ERR_INVALID and needle in msg, (rc, msg)


def test_alg_plan_names_the_missing_head_key():
    rc, msg = _create(_cfg(model=H.LT_MODEL_ALG))
    assert rc == ERR_INVALID and "backbone.final_layer.weight" in msg, msg
    rc, msg = _create(_cfg(model=H.LT_MODEL_ALG, use_confidences=1), ("backbone.final_layer.weight", "backbone.final_layer.bias"))
    assert rc == ERR_INVALID and "backbone.alg_confidences.head.4.weight" in msg, msg
    rc, msg = _create(_cfg(model=H.LT_MODEL_RANSAC), ("module.backbone.final_layer.weight",))          # "module." is stripped
    assert rc == ERR_INVALID and "backbone.final_layer.bias" in msg, msg


def test_alg_tail_kernel_argument_checks():
    lib = H.lib()
    assert lib.lt_alg_tail_fwd(None, None, 17, 1, 1.0, 1.0, None, None, 1, 2, 4, 17, None) == ERR_INVALID and "null" in lib.lt_last_error().decode()
    assert lib.lt_alg_tail_fwd(1, None, 17, 1, 1.0, 1.0, None, None, 1, 2, 1, 17, None) == ERR_INVALID and b"NV 1" in lib.lt_last_error()
    assert lib.lt_alg_tail_fwd(1, 1, 16, 1, 1.0, 1.0, None, None, 1, 2, 4, 17, None) == ERR_INVALID and b"ld_conf 16" in lib.lt_last_error()
