"""CPU: lt_unproject_desc and its three entries (include/lt_hip.h) -- the symbols, the struct's layout as ctypes sees it, the rules for which pointer
patterns are a variant and which have no kernel, the workspace query against the two shorthand queries, and the name helper.  No device work: every
argument check of the library precedes its first device call, so a pointer here is only ever tested for being set (the value 1)."""
import ctypes as C
import itertools
import os
import re

import pytest

import lt_hip as H
import unproject_bwd_indexed_ref as X
from mvn.utils import op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lt_unproject_desc_fwd", "lt_unproject_desc_bwd_workspace", "lt_unproject_desc_bwd")
INVALID, UNSUPPORTED = -1, -2
CUBOID = dict(pos=1, center=1, rot=1, coords_out=1)


def _desc(**over):
    """A descriptor that passes every check of both entries: the coordinate form, plain, fp32."""
    kw = dict(dtype=H.LT_F32, feats=1, proj=1, coords=1, B=2, NV=3, C=4, h=12, w=16, v0=5, v1=6, v2=7, agg=H.AGG["softmax"])
    kw.update(over)
    return H.UnprojectDesc(**kw)


def _fwd(d):
    lib = H.lib()
    return lib.lt_unproject_desc_fwd(C.byref(d), 1, None), lib.lt_last_error().decode()


def _bwd(d, ws_bytes=0):
    lib = H.lib()
    return lib.lt_unproject_desc_bwd(C.byref(d), 1, 1, 1, None, ws_bytes, None), lib.lt_last_error().decode()


def test_the_three_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lt_hip.h")).read(), flags=re.S)
    raw = C.CDLL(H.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared"
        assert hasattr(raw, name), name + " is not exported"
        assert name in H.SIGNATURES and getattr(H.lib(), name).argtypes[0] == C.POINTER(H.UnprojectDesc), name + " is not bound"
    assert "typedef struct lt_unproject_desc" in hdr and H.lib().lt_abi_version() == 1
    assert H.UnprojectDesc._fields_[-1][0] == "agg" and H.UnprojectDesc._fields_[0][0] == "dtype"


def test_struct_layout_end_to_end_last_and_first_field():
    """agg is the struct's LAST field and dtype its first: a descriptor that is valid but for one of them is refused with that field's value in the
    message, so both ends of the layout (and every offset between them, through the checks that pass) are what the library reads."""
    rc, msg = _fwd(_desc(agg=9))
    assert rc == INVALID and "aggregation 9" in msg, (rc, msg)
    rc, msg = _fwd(_desc(dtype=7))
    assert rc == INVALID and "dtype 7" in msg, (rc, msg)
    # the valid descriptor passes every check of the backward up to the workspace, whose message states the query's own number
    d = _desc()
    rc, msg = _bwd(d)
    assert rc == INVALID and "workspace of at least %d bytes" % H.lib().lt_unproject_desc_bwd_workspace(C.byref(d), 1) in msg, (rc, msg)
    assert H.lib().lt_unproject_desc_fwd(None, 1, None) == INVALID and b"null descriptor" in H.lib().lt_last_error()
    assert H.lib().lt_unproject_desc_bwd(None, 1, 1, 1, None, 0, None) == INVALID and b"null descriptor" in H.lib().lt_last_error()


@pytest.mark.parametrize("over,code,words", [
    (dict(view_base=1, T=6, view_mask=1), UNSUPPORTED, ("view_base", "view_mask")),
    (dict(view_base=1, T=6, frame_of=1, F=2), UNSUPPORTED, ("view_base", "frame_of")),
    (dict(CUBOID), INVALID, ("both", "coords", "cuboid")),
    (dict(coords=None), INVALID, ("neither", "coords", "cuboid")),
    (dict(coords=None, pos=1, center=1, rot=1), INVALID, ("null argument",)),          # a cuboid without its coords_out
    (dict(coords=None, v1=5, v2=5, agg=9, **CUBOID), INVALID, ("aggregation 9",)),      # the grid form, V cubed, is a variant: it gets as far as the aggregation
    (dict(coords=None, **CUBOID), INVALID, ("bad shape",)),                             # ... and needs v0 = v1 = v2
    (dict(view_base=1, T=0), INVALID, ("T 0 images",)),
    (dict(view_base=1, T=6, NV=33), INVALID, ("NVcap 33",)),
    (dict(frame_of=1, F=0), INVALID, ("F 0 frames",)),
], ids=["ragged+mask", "ragged+indexed", "coords+cuboid", "neither", "half_a_cuboid", "grid", "grid_not_a_cube", "ragged_T", "ragged_NVcap", "indexed_F"])
def test_forward_combination_rules(over, code, words):
    rc, msg = _fwd(_desc(**over))
    assert rc == code and msg.startswith("lt_unproject_desc_fwd:") and all(w in msg for w in words), (rc, msg)


@pytest.mark.parametrize("over,code,words", [
    (dict(view_base=1, T=6), UNSUPPORTED, ("view_base", "backward")),
    (dict(view_base=1, T=6, view_mask=1), UNSUPPORTED, ("view_base", "backward")),
    (dict(CUBOID), INVALID, ("both", "coords", "cuboid")),
    (dict(coords=None), INVALID, ("null argument",)),
    (dict(frame_of=1, F=0), INVALID, ("F >= 1 frames", "F=0 P=2")),
    (dict(view_mask=1, C=48), UNSUPPORTED, ("view mask", "C=48", "no masked form")),
    (dict(frame_of=1, F=2, C=48), UNSUPPORTED, ("frame index", "C=48", "no indexed form")),
    (dict(frame_of=1, F=2, view_mask=1, C=48), UNSUPPORTED, ("frame index", "C=48", "no indexed form")),
    (dict(agg=9), UNSUPPORTED, ("aggregation 9",)),
    (dict(NV=33), UNSUPPORTED, ("NV=33",)),
], ids=["ragged", "ragged+mask", "coords+cuboid", "no_coords", "indexed_F", "masked_scatter", "indexed_scatter", "indexed+mask_scatter", "agg", "NV"])
def test_backward_combination_rules(over, code, words):
    rc, msg = _bwd(_desc(**over))
    assert rc == code and msg.startswith("lt_unproject_desc_bwd:") and all(w in msg for w in words), (rc, msg)


def test_backward_reads_the_grid_forms_coords_out():
    """A descriptor in the grid form is shared by a forward and its backward: the backward reads the coords_out the forward wrote, so it passes the
    null-argument check and stops at the workspace."""
    rc, msg = _bwd(_desc(coords=None, v1=5, v2=5, **CUBOID))
    assert rc == INVALID and "workspace of at least" in msg, (rc, msg)


@pytest.mark.parametrize("vs", [(4, 4, 16), (5, 6, 7), (16, 16, 16)], ids=lambda v: "x".join(map(str, v)))
def test_workspace_query_agrees_with_the_shorthand_queries(vs):
    lib, P = H.lib(), 5
    for Cc, NV in itertools.product((4, 8, 32, 64, 48), (1, 4, 9, 32)):
        plain, masked = _desc(B=P, NV=NV, C=Cc, v0=vs[0], v1=vs[1], v2=vs[2]), _desc(B=P, NV=NV, C=Cc, v0=vs[0], v1=vs[1], v2=vs[2], view_mask=1)
        indexed = _desc(B=P, NV=NV, C=Cc, v0=vs[0], v1=vs[1], v2=vs[2], frame_of=1, F=2)
        both = _desc(B=P, NV=NV, C=Cc, v0=vs[0], v1=vs[1], v2=vs[2], frame_of=1, F=2, view_mask=1)
        whole = lib.lt_unproject_indexed_bwd_workspace(P, NV, Cc, *vs)
        assert (whole == 0) == (Cc == 48) == (lib.lt_unproject_bwd_workspace(P, NV, Cc, *vs) == 0), (Cc, NV, whole)
        for items in (1, 2, P):
            q = lambda d: lib.lt_unproject_desc_bwd_workspace(C.byref(d), items)
            # plain and masked: `items` samples' shares, partials included, which is the shorthand query of a batch of `items`
            assert q(plain) == q(masked) == lib.lt_unproject_bwd_workspace(items, NV, Cc, *vs), (Cc, NV, items)
            # indexed, with or without a mask: the partials of all P cuboids plus `items` shares, stated twice independently of the new query
            # (X.ws_bytes restates the header's formula over the shorthand query) and through op, which asks the library
            assert q(indexed) == q(both) == X.ws_bytes(lib, P, NV, Cc, vs, items) == op.indexed_bwd_workspace(P, NV, Cc, *vs, chunk=items), (Cc, NV, items)
        assert lib.lt_unproject_desc_bwd_workspace(C.byref(indexed), P) == whole == op.indexed_bwd_workspace(P, NV, Cc, *vs)
        assert lib.lt_unproject_desc_bwd_workspace(C.byref(plain), 0) == 0 and lib.lt_unproject_desc_bwd_workspace(C.byref(plain), P + 3) == \
            lib.lt_unproject_bwd_workspace(P, NV, Cc, *vs)
        assert lib.lt_unproject_desc_bwd_workspace(C.byref(_desc(B=P, NV=NV, C=Cc, view_base=1, T=6)), 1) == 0          # no ragged backward
        # op.unproject_bwd_workspace: the cap picks the largest chunk that fits, at least one
        if whole:
            for d, legacy in ((plain, lambda k: lib.lt_unproject_bwd_workspace(k, NV, Cc, *vs)), (indexed, lambda k: X.ws_bytes(lib, P, NV, Cc, vs, k))):
                assert op.unproject_bwd_workspace(d) == legacy(P) and op.unproject_bwd_workspace(d, chunk=2) == legacy(2)
                assert op.unproject_bwd_workspace(d, cap=legacy(2) + 100) == legacy(2) and op.unproject_bwd_workspace(d, cap=0) == legacy(1)
                assert op.unproject_bwd_workspace(d, cap=1 << 62) == legacy(P)
        else:
            assert op.unproject_bwd_workspace(plain, cap=1 << 30) == 0 == op.unproject_bwd_workspace(indexed)


def test_variant_name_helper_names_the_eight_forward_entries_and_the_three_backward_ones():
    variants = {"": {}, "_masked": dict(view_mask=1), "_indexed": dict(frame_of=1, F=2), "_ragged": dict(view_base=1, T=6)}
    names = set()
    for (form, fkw), (variant, vkw) in itertools.product((("", dict(coords=1)), ("_grid", dict(coords=None, **CUBOID))), variants.items()):
        name = H.unproject_entry(_desc(**fkw, **vkw))
        assert name == "lt_unproject%s%s_fwd" % (form, variant) and name in H.SIGNATURES, name
        names.add(name)
    assert len(names) == 8
    # a frame index makes it the indexed entry whether or not there is a mask, as in the library's own choice of the instantiation
    assert H.unproject_entry(_desc(frame_of=1, F=2, view_mask=1)) == "lt_unproject_indexed_fwd"
    for variant, vkw in list(variants.items())[:3]:
        for fkw in (dict(coords=1), dict(coords=None, **CUBOID)):          # the backward has no grid entry: a shared grid descriptor names the same one
            name = H.unproject_entry(_desc(**fkw, **vkw), bwd=True)
            assert name == "lt_unproject%s_bwd" % variant and name in H.SIGNATURES, name
