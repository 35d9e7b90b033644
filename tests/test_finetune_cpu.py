"""No GPU: the argument rules of lt_bn_act_bwd with optional outputs (fine-tuning with frozen parameters).  dgamma / dbeta are given together or not
at all (frozen affine parameters), dy may be left out when only the parameter gradients are wanted (then dy_bf16 and dres are left out too), and the
shape check comes in front of the optional-pointer checks -- every refusal here returns before anything is launched."""
import lt_hip as H

ERR_INVALID = -1
P = 64          # a dummy non-null pointer: every case below is refused before it would be read


def _call(lib, dy=P, dy16=None, dgamma=P, dbeta=P, dres=None, res=None, rows=8, C=16, flags=0, ws=P):
    return lib.lt_bn_act_bwd(P, P, res, P, P, P, P, dy, dy16, dgamma, dbeta, dres, 0, rows, C, 1e-5, flags, ws, None)


def test_bn_act_bwd_checks_the_shape_before_the_optional_outputs():
    lib = H.lib()
    err = lambda: lib.lt_last_error().decode()
    assert _call(lib, dgamma=None, dbeta=None, rows=0) == ERR_INVALID
    assert "bad shape" in err() and "rows=0" in err() and "C=16" in err(), err()
    assert _call(lib, dgamma=None, dbeta=None, C=4097) == ERR_INVALID and "C=4097" in err()
    # the inputs stay mandatory
    assert lib.lt_bn_act_bwd(None, P, None, P, P, P, P, P, None, P, P, None, 0, 8, 16, 1e-5, 0, P, None) == ERR_INVALID and "null argument" in err()


def test_bn_act_bwd_wants_dgamma_and_dbeta_together():
    lib = H.lib()
    err = lambda: lib.lt_last_error().decode()
    assert _call(lib, dgamma=None) == ERR_INVALID
    assert "dgamma" in err() and "dbeta" in err() and "together" in err(), err()
    assert "dgamma NULL, dbeta given" in err()
    assert _call(lib, dbeta=None) == ERR_INVALID and "dgamma given, dbeta NULL" in err()
    assert _call(lib, dbeta=None, flags=H.BN_FROZEN) == ERR_INVALID and "together" in err()


def test_bn_act_bwd_refuses_a_call_without_any_output():
    lib = H.lib()
    err = lambda: lib.lt_last_error().decode()
    assert _call(lib, dy=None, dgamma=None, dbeta=None) == ERR_INVALID and "no output" in err(), err()
    assert _call(lib, dy=None, dgamma=None, dbeta=None, flags=H.BN_FROZEN) == ERR_INVALID and "no output" in err()


def test_bn_act_bwd_without_dy_takes_no_dres_and_no_bf16_copy():
    lib = H.lib()
    err = lambda: lib.lt_last_error().decode()
    assert _call(lib, dy=None, dres=P, res=P) == ERR_INVALID and "without dy" in err() and "dres" in err(), err()
    assert _call(lib, dy=None, dy16=P) == ERR_INVALID and "without dy" in err() and "dy_bf16" in err()
    # ... and the older rules hold: a residual gradient needs the residual; only the elementwise case runs without a workspace
    assert _call(lib, dres=P, res=None) == ERR_INVALID and "needs the residual" in err()
    assert _call(lib, ws=None) == ERR_INVALID and "workspace" in err()
    assert _call(lib, dgamma=None, dbeta=None, ws=None) == ERR_INVALID and "workspace" in err()          # batch statistics: the sums go to the workspace


def test_bn_act_bwd_workspace_holds_the_finalized_sums():
    """2 C floats behind the fp64 partial sums, for a call with batch statistics and without dgamma / dbeta."""
    lib = H.lib()
    for rows, C in ((37, 4), (515, 64), (96, 17), (33, 1028), (70000, 32)):
        need = lib.lt_bn_act_bwd_workspace(rows, C)
        assert need >= 16 * C + 8 * C and need % 4 == 0, (rows, C, need)          # >= one slab of partials (2 doubles per channel) + 2 C floats
