"""CPU: the plan's kernel-selection rules (csrc/select.hip, called by both plan hosts) on shapes on both sides of every threshold, with each A/B switch
unset and set.  The expected answers were frozen from the rules as the two hosts restated them before the library owned them; a switch set to "0" or
to the empty string is off, i.e. answers as if it were unset."""
import os

import pytest
import torch

import lt_engine as E

def W(*s):          # the rules read shapes only: large weights stay on the meta device
    return torch.zeros(s) if len(s) and s[0] * s[1] <= 256 * 256 else torch.empty(s, device="meta")

class A:
    def __init__(self, *s): self.shape = tuple(s)

B1 = [(64, 256, 1, 1), (64, 64, 3, 3), (256, 64, 1, 1)]
B2 = [(128, 512, 1, 1), (128, 128, 3, 3), (512, 128, 1, 1)]
B3 = [(256, 1024, 1, 1), (256, 256, 3, 3), (1024, 256, 1, 1)]
DS = [(64, 64, 1, 1), (64, 64, 3, 3), (256, 64, 1, 1)]

def cases():
    c = []
    for n, d, h, w in [(1, 64, 64, 64), (3, 64, 64, 64), (4, 64, 64, 64), (15, 32, 32, 32), (16, 32, 32, 32), (16, 4, 32, 32), (16, 8, 32, 32),
                       (16, 32, 36, 32), (63, 2048, 16, 16), (100, 2048, 16, 16), (248, 2048, 16, 16), (249, 2048, 16, 16)]:
        c.append(("conv_skip", (n, d, h, w)))
    c.append(("conv_skip_w", None))
    for (P, Cc, Cin2, Ho, s) in [(128, 512, 256, 48, 2), (512, 2048, 1024, 12, 2), (64, 256, 64, 96, 1), (256, 1024, 512, 24, 2), (96, 512, 256, 48, 2),
                                 (128, 512, 256, 48, 3)]:
        for n in (1, 12, 13, 48, 49, 64):
            c.append(("cat2", (n, P, Cc, Cin2, Ho, s)))
    for V, cin in [(8, 128), (4, 128), (2, 128), (16, 128), (8, 64), (8, 192)]:
        for n in (1, 2, 3, 4, 5, 8, 16, 32, 64):
            c.append(("splitk", (n, V, cin)))
    for n in (1, 5):
        for k, blk in (("b1", B1), ("b2", B2), ("b3", B3)):
            for h, w in ((96, 96), (48, 48), (24, 24), (12, 24), (16, 40), (96, 8)):
                cin = blk[0][1]
                c.append(("bneck", (k, n, h, w, cin)))
        for h, w, sd in ((96, 96, 1), (96, 96, 2), (92, 96, 1), (96, 88, 1)):
            c.append(("bneck_ds", (n, h, w, sd)))
    for n in (1, 2, 5, 6, 64):
        for h, w in ((24, 24), (24, 144), (12, 12)):
            c.append(("xr", (n, h, w)))
    for cin, k, s, p, pool in ((8, 7, 2, 3, (3, 2, 1)), (16, 7, 2, 3, (3, 2, 1)), (8, 5, 2, 3, (3, 2, 1)), (8, 7, 2, 3, (3, 2, 0))):
        c.append(("stem", (cin, k, s, p, pool)))
    for vox, widths in (((32, 32, 32), (32, 32, 17)), ((32, 32, 31), (32, 32, 17)), ((4, 4, 4), (32, 17)), ((8, 8, 8), (32, 64, 17)), ((8, 8, 8), (33,))):
        c.append(("pwchain", (vox, widths)))
    # layouts: (kind, N, H, W, cin, cout, transposed, stride, pad, residual, out_f32, dtype)
    L = []
    for n in (1, 4, 5, 19, 20, 64):
        L += [("2d", n, 24, 24, 256, 256, 3, False, 1, 1, False, False), ("2d", n, 48, 48, 256, 256, 3, False, 1, 1, False, False),
              ("2d", n, 24, 24, 256, 256, 4, True, 2, 1, False, False), ("2d", n, 48, 48, 256, 256, 4, True, 2, 1, False, False),
              ("2d", n, 12, 12, 2048, 256, 4, True, 2, 1, False, False)]
    for n in (5, 20):
        L += [("2d", n, 24, 24, 256, 256, 3, False, 1, 1, True, False), ("2d", n, 24, 24, 256, 256, 3, False, 1, 1, False, True),
              ("2d", n, 24, 24, 1024, 256, 1, False, 1, 0, False, False), ("2d", n, 24, 24, 256, 1024, 1, False, 1, 0, False, False),
              ("2d", n, 96, 96, 64, 256, 1, False, 1, 0, False, False), ("2d", n, 96, 96, 64, 64, 3, False, 1, 1, False, False),
              ("2d", n, 48, 48, 256, 512, 1, False, 2, 0, False, False)]
    for n in (1, 4):
        for ci, co in ((64, 64), (32, 64), (128, 128), (16, 32), (32, 32), (64, 128)):
            L += [("3d", n, 16, 16, ci, co, 3, False, 1, 1, False, False)]
        L += [("3d", n, 16, 16, 32, 64, 3, False, 2, 1, False, False), ("3d", n, 16, 16, 64, 64, 2, True, 2, 0, False, False)]
    for l in L:
        c.append(("layout", l))
    return c


BLK = {"b1": B1, "b2": B2, "b3": B3}
ENVS = {"conv_skip": ["LT_NO_CONV_SKIP", "LT_HALO_NO_COL", "LT_HALO_NO_PERSIST", "LT_CONV_NO_HALO"], "conv_skip_w": [],
        "cat2": ["LT_NO_CONV_CAT2", "LT_CONV_NO_V7", "LT_CONV_NO_V3", "LT_CAT2_ANY_SIZE"], "splitk": ["LT_CONV_NO_SPLITK"],
        "bneck": ["LT_NO_BNECK"], "bneck_ds": ["LT_NO_BNECK", "LT_NO_BNECK_DS"], "xr": ["LT_NO_XR", "LT_XR_ANY_SIZE"], "stem": [], "pwchain": [],
        "layout": ["LT_CONV_NO_H2D", "LT_CONV_V1", "LT_H2D_ANY_SIZE", "LT_DECONV_NO_H2D", "LT_CONV_NO_V7"]}

def layout_spec(a):
    kind, n, h, w, ci, co, k, tr, s, p, res, f32 = a
    if kind == "2d":
        wt = W(ci, co, k, k) if tr else W(co, ci, k, k)
        xs = (n, 1, h, w, ci)
    else:
        wt = W(ci, co, k, k, k) if tr else W(co, ci, k, k, k)
        xs = (n, h, h, w, ci)
    wt = torch.zeros(wt.shape)
    spec = E.make_conv_spec(wt, None, None, xs, s, p, torch.bfloat16, tr, E.H.EPI_STORE_F32 if f32 else 0)
    return spec, wt, tr, res

def ev(pb, rule, a, layout_fn):
    if rule == "conv_skip":
        n, d, h, w = a
        return pb.can_conv_skip((n, d, h, w, 32), W(32, 32, 3, 3, 3), (n, d, h, w, 16), W(32, 16, 1, 1, 1))
    if rule == "conv_skip_w":
        return (pb.can_conv_skip((4, 64, 64, 64, 32), W(32, 32, 3, 3, 3), (4, 64, 64, 64, 16), W(32, 16, 3, 3, 3)),
                pb.can_conv_skip((4, 64, 64, 64, 32), W(64, 32, 3, 3, 3), (4, 64, 64, 64, 16), W(32, 16, 1, 1, 1)))
    if rule == "cat2":
        n, P, Cc, Cin2, Ho, s = a
        return pb.can_conv_cat2((n, 1, Ho, Ho, P), W(Cc, P, 1, 1), (n, 1, Ho * s, Ho * s, Cin2), W(Cc, Cin2, 1, 1), s)
    if rule == "splitk":
        n, V, cin = a
        wt = torch.zeros(128, cin, 3, 3, 3)
        spec = E.make_conv_spec(wt, None, None, (n, V, V, V, cin), 1, 1, torch.bfloat16)
        return pb.splitk_slices(spec, wt, False, False, False, None)
    if rule == "bneck":
        k, n, h, w, cin = a
        return pb.can_bottleneck(A(n, 1, h, w, cin), [W(*s) for s in BLK[k]], (1, 1, 1))
    if rule == "bneck_ds":
        n, h, w, sd = a
        return pb.can_bottleneck_ds(A(n, 1, h, w, 64), [W(*s) for s in DS], (1, 1, 1), W(256, 64, 1, 1), sd)
    if rule == "xr":
        n, h, w = a
        return pb.can_expand_reduce(A(n, 1, h, w, 256), A(n, 1, h, w, 1024), W(1024, 256, 1, 1), W(256, 1024, 1, 1))
    if rule == "stem":
        cin, k, s, p, pool = a
        return pb.can_stem_pool(A(2, 1, 64, 64, cin), W(64, 3, k, k), s, p, pool)
    if rule == "pwchain":
        vox, widths = a
        layers, cin = [], 32
        for co in widths:
            layers.append((W(co, cin, 1, 1, 1), None, None, True)); cin = co
        return pb.can_chain_pointwise(A(2, *vox, 32), layers)
    if rule == "layout":
        return layout_fn(pb, *layout_spec(a))


EXPECTED = {
    ('conv_skip', (1, 64, 64, 64)): (False, False, False, False, False, False),
    ('conv_skip', (3, 64, 64, 64)): (False, False, False, False, False, False),
    ('conv_skip', (4, 64, 64, 64)): (True, False, False, False, False, False),
    ('conv_skip', (15, 32, 32, 32)): (False, False, False, False, False, False),
    ('conv_skip', (16, 32, 32, 32)): (True, False, False, False, False, False),
    ('conv_skip', (16, 4, 32, 32)): (False, False, False, False, False, False),
    ('conv_skip', (16, 8, 32, 32)): (False, False, False, False, False, False),
    ('conv_skip', (16, 32, 36, 32)): (False, False, False, False, False, False),
    ('conv_skip', (63, 2048, 16, 16)): (False, False, False, False, False, False),
    ('conv_skip', (100, 2048, 16, 16)): (True, False, False, False, False, False),
    ('conv_skip', (248, 2048, 16, 16)): (True, False, False, False, False, False),
    ('conv_skip', (249, 2048, 16, 16)): (False, False, False, False, False, False),
    ('conv_skip_w', None): ((False, False), (False, False)),
    ('cat2', (1, 128, 512, 256, 48, 2)): (False, False, False, False, True, False),
    ('cat2', (12, 128, 512, 256, 48, 2)): (False, False, False, False, True, False),
    ('cat2', (13, 128, 512, 256, 48, 2)): (True, False, False, False, True, False),
    ('cat2', (48, 128, 512, 256, 48, 2)): (True, False, False, False, True, False),
    ('cat2', (49, 128, 512, 256, 48, 2)): (True, False, False, False, True, False),
    ('cat2', (64, 128, 512, 256, 48, 2)): (True, False, False, False, True, False),
    ('cat2', (1, 512, 2048, 1024, 12, 2)): (False, False, False, False, True, False),
    ('cat2', (12, 512, 2048, 1024, 12, 2)): (False, False, False, False, True, False),
    ('cat2', (13, 512, 2048, 1024, 12, 2)): (False, False, False, False, True, False),
    ('cat2', (48, 512, 2048, 1024, 12, 2)): (False, False, False, False, True, False),
    ('cat2', (49, 512, 2048, 1024, 12, 2)): (True, False, False, False, True, False),
    ('cat2', (64, 512, 2048, 1024, 12, 2)): (True, False, False, False, True, False),
    ('cat2', (1, 64, 256, 64, 96, 1)): (False, False, False, False, True, False),
    ('cat2', (12, 64, 256, 64, 96, 1)): (True, False, False, False, True, False),
    ('cat2', (13, 64, 256, 64, 96, 1)): (True, False, False, False, True, False),
    ('cat2', (48, 64, 256, 64, 96, 1)): (True, False, False, False, True, False),
    ('cat2', (49, 64, 256, 64, 96, 1)): (True, False, False, False, True, False),
    ('cat2', (64, 64, 256, 64, 96, 1)): (True, False, False, False, True, False),
    ('cat2', (1, 256, 1024, 512, 24, 2)): (False, False, False, False, True, False),
    ('cat2', (12, 256, 1024, 512, 24, 2)): (False, False, False, False, True, False),
    ('cat2', (13, 256, 1024, 512, 24, 2)): (False, False, False, False, True, False),
    ('cat2', (48, 256, 1024, 512, 24, 2)): (True, False, False, False, True, False),
    ('cat2', (49, 256, 1024, 512, 24, 2)): (True, False, False, False, True, False),
    ('cat2', (64, 256, 1024, 512, 24, 2)): (True, False, False, False, True, False),
    ('cat2', (1, 96, 512, 256, 48, 2)): (False, False, False, False, False, False),
    ('cat2', (12, 96, 512, 256, 48, 2)): (False, False, False, False, False, False),
    ('cat2', (13, 96, 512, 256, 48, 2)): (False, False, False, False, False, False),
    ('cat2', (48, 96, 512, 256, 48, 2)): (False, False, False, False, False, False),
    ('cat2', (49, 96, 512, 256, 48, 2)): (False, False, False, False, False, False),
    ('cat2', (64, 96, 512, 256, 48, 2)): (False, False, False, False, False, False),
    ('cat2', (1, 128, 512, 256, 48, 3)): (False, False, False, False, False, False),
    ('cat2', (12, 128, 512, 256, 48, 3)): (False, False, False, False, False, False),
    ('cat2', (13, 128, 512, 256, 48, 3)): (False, False, False, False, False, False),
    ('cat2', (48, 128, 512, 256, 48, 3)): (False, False, False, False, False, False),
    ('cat2', (49, 128, 512, 256, 48, 3)): (False, False, False, False, False, False),
    ('cat2', (64, 128, 512, 256, 48, 3)): (False, False, False, False, False, False),
    ('splitk', (1, 8, 128)): (8, 1, 1),
    ('splitk', (2, 8, 128)): (8, 1, 1),
    ('splitk', (3, 8, 128)): (5, 1, 1),
    ('splitk', (4, 8, 128)): (4, 1, 1),
    ('splitk', (5, 8, 128)): (3, 1, 1),
    ('splitk', (8, 8, 128)): (2, 1, 1),
    ('splitk', (16, 8, 128)): (4, 1, 1),
    ('splitk', (32, 8, 128)): (2, 1, 1),
    ('splitk', (64, 8, 128)): (1, 1, 1),
    ('splitk', (1, 4, 128)): (8, 1, 1),
    ('splitk', (2, 4, 128)): (8, 1, 1),
    ('splitk', (3, 4, 128)): (8, 1, 1),
    ('splitk', (4, 4, 128)): (8, 1, 1),
    ('splitk', (5, 4, 128)): (8, 1, 1),
    ('splitk', (8, 4, 128)): (8, 1, 1),
    ('splitk', (16, 4, 128)): (8, 1, 1),
    ('splitk', (32, 4, 128)): (4, 1, 1),
    ('splitk', (64, 4, 128)): (2, 1, 1),
    ('splitk', (1, 2, 128)): (8, 1, 1),
    ('splitk', (2, 2, 128)): (8, 1, 1),
    ('splitk', (3, 2, 128)): (8, 1, 1),
    ('splitk', (4, 2, 128)): (8, 1, 1),
    ('splitk', (5, 2, 128)): (8, 1, 1),
    ('splitk', (8, 2, 128)): (8, 1, 1),
    ('splitk', (16, 2, 128)): (8, 1, 1),
    ('splitk', (32, 2, 128)): (8, 1, 1),
    ('splitk', (64, 2, 128)): (8, 1, 1),
    ('splitk', (1, 16, 128)): (1, 1, 1),
    ('splitk', (2, 16, 128)): (1, 1, 1),
    ('splitk', (3, 16, 128)): (1, 1, 1),
    ('splitk', (4, 16, 128)): (1, 1, 1),
    ('splitk', (5, 16, 128)): (1, 1, 1),
    ('splitk', (8, 16, 128)): (1, 1, 1),
    ('splitk', (16, 16, 128)): (1, 1, 1),
    ('splitk', (32, 16, 128)): (1, 1, 1),
    ('splitk', (64, 16, 128)): (1, 1, 1),
    ('splitk', (1, 8, 64)): (1, 1, 1),
    ('splitk', (2, 8, 64)): (1, 1, 1),
    ('splitk', (3, 8, 64)): (1, 1, 1),
    ('splitk', (4, 8, 64)): (1, 1, 1),
    ('splitk', (5, 8, 64)): (1, 1, 1),
    ('splitk', (8, 8, 64)): (1, 1, 1),
    ('splitk', (16, 8, 64)): (1, 1, 1),
    ('splitk', (32, 8, 64)): (1, 1, 1),
    ('splitk', (64, 8, 64)): (1, 1, 1),
    ('splitk', (1, 8, 192)): (8, 1, 1),
    ('splitk', (2, 8, 192)): (8, 1, 1),
    ('splitk', (3, 8, 192)): (5, 1, 1),
    ('splitk', (4, 8, 192)): (4, 1, 1),
    ('splitk', (5, 8, 192)): (3, 1, 1),
    ('splitk', (8, 8, 192)): (2, 1, 1),
    ('splitk', (16, 8, 192)): (4, 1, 1),
    ('splitk', (32, 8, 192)): (2, 1, 1),
    ('splitk', (64, 8, 192)): (1, 1, 1),
    ('bneck', ('b1', 1, 96, 96, 256)): (True, False, False),
    ('bneck', ('b1', 1, 48, 48, 256)): (True, False, False),
    ('bneck', ('b1', 1, 24, 24, 256)): (False, False, False),
    ('bneck', ('b1', 1, 12, 24, 256)): (False, False, False),
    ('bneck', ('b1', 1, 16, 40, 256)): (False, False, False),
    ('bneck', ('b1', 1, 96, 8, 256)): (False, False, False),
    ('bneck', ('b2', 1, 96, 96, 512)): (True, False, False),
    ('bneck', ('b2', 1, 48, 48, 512)): (True, False, False),
    ('bneck', ('b2', 1, 24, 24, 512)): (False, False, False),
    ('bneck', ('b2', 1, 12, 24, 512)): (False, False, False),
    ('bneck', ('b2', 1, 16, 40, 512)): (False, False, False),
    ('bneck', ('b2', 1, 96, 8, 512)): (False, False, False),
    ('bneck', ('b3', 1, 96, 96, 1024)): (False, False, False),
    ('bneck', ('b3', 1, 48, 48, 1024)): (False, False, False),
    ('bneck', ('b3', 1, 24, 24, 1024)): (False, False, False),
    ('bneck', ('b3', 1, 12, 24, 1024)): (False, False, False),
    ('bneck', ('b3', 1, 16, 40, 1024)): (False, False, False),
    ('bneck', ('b3', 1, 96, 8, 1024)): (False, False, False),
    ('bneck_ds', (1, 96, 96, 1)): (True, False, False, False),
    ('bneck_ds', (1, 96, 96, 2)): (False, False, False, False),
    ('bneck_ds', (1, 92, 96, 1)): (False, False, False, False),
    ('bneck_ds', (1, 96, 88, 1)): (False, False, False, False),
    ('bneck', ('b1', 5, 96, 96, 256)): (True, False, False),
    ('bneck', ('b1', 5, 48, 48, 256)): (True, False, False),
    ('bneck', ('b1', 5, 24, 24, 256)): (False, False, False),
    ('bneck', ('b1', 5, 12, 24, 256)): (False, False, False),
    ('bneck', ('b1', 5, 16, 40, 256)): (False, False, False),
    ('bneck', ('b1', 5, 96, 8, 256)): (False, False, False),
    ('bneck', ('b2', 5, 96, 96, 512)): (True, False, False),
    ('bneck', ('b2', 5, 48, 48, 512)): (True, False, False),
    ('bneck', ('b2', 5, 24, 24, 512)): (False, False, False),
    ('bneck', ('b2', 5, 12, 24, 512)): (False, False, False),
    ('bneck', ('b2', 5, 16, 40, 512)): (False, False, False),
    ('bneck', ('b2', 5, 96, 8, 512)): (False, False, False),
    ('bneck', ('b3', 5, 96, 96, 1024)): (False, False, False),
    ('bneck', ('b3', 5, 48, 48, 1024)): (False, False, False),
    ('bneck', ('b3', 5, 24, 24, 1024)): (False, False, False),
    ('bneck', ('b3', 5, 12, 24, 1024)): (False, False, False),
    ('bneck', ('b3', 5, 16, 40, 1024)): (False, False, False),
    ('bneck', ('b3', 5, 96, 8, 1024)): (False, False, False),
    ('bneck_ds', (5, 96, 96, 1)): (True, False, False, False),
    ('bneck_ds', (5, 96, 96, 2)): (False, False, False, False),
    ('bneck_ds', (5, 92, 96, 1)): (False, False, False, False),
    ('bneck_ds', (5, 96, 88, 1)): (False, False, False, False),
    ('xr', (1, 24, 24)): (False, False, True, False),
    ('xr', (1, 24, 144)): (True, False, True, False),
    ('xr', (1, 12, 12)): (False, False, True, False),
    ('xr', (2, 24, 24)): (False, False, True, False),
    ('xr', (2, 24, 144)): (True, False, True, False),
    ('xr', (2, 12, 12)): (False, False, True, False),
    ('xr', (5, 24, 24)): (False, False, True, False),
    ('xr', (5, 24, 144)): (True, False, True, False),
    ('xr', (5, 12, 12)): (False, False, True, False),
    ('xr', (6, 24, 24)): (True, False, True, False),
    ('xr', (6, 24, 144)): (True, False, True, False),
    ('xr', (6, 12, 12)): (False, False, True, False),
    ('xr', (64, 24, 24)): (True, False, True, False),
    ('xr', (64, 24, 144)): (True, False, True, False),
    ('xr', (64, 12, 12)): (True, False, True, False),
    ('stem', (8, 7, 2, 3, (3, 2, 1))): (True, False),
    ('stem', (16, 7, 2, 3, (3, 2, 1))): (False, False),
    ('stem', (8, 5, 2, 3, (3, 2, 1))): (False, False),
    ('stem', (8, 7, 2, 3, (3, 2, 0))): (False, False),
    ('pwchain', ((32, 32, 32), (32, 32, 17))): (True, False),
    ('pwchain', ((32, 32, 31), (32, 32, 17))): (True, False),
    ('pwchain', ((4, 4, 4), (32, 17))): (True, False),
    ('pwchain', ((8, 8, 8), (32, 64, 17))): (False, False),
    ('pwchain', ((8, 8, 8), (33,))): (False, False),
    ('layout', ('2d', 1, 24, 24, 256, 256, 3, False, 1, 1, False, False)): (3, 3, 3, 2, 3, 1),
    ('layout', ('2d', 1, 48, 48, 256, 256, 3, False, 1, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 1, 24, 24, 256, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 2, 3, 1),
    ('layout', ('2d', 1, 48, 48, 256, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 2, 3, 1),
    ('layout', ('2d', 1, 12, 12, 2048, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 4, 24, 24, 256, 256, 3, False, 1, 1, False, False)): (3, 3, 3, 2, 3, 1),
    ('layout', ('2d', 4, 48, 48, 256, 256, 3, False, 1, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 4, 24, 24, 256, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 2, 3, 1),
    ('layout', ('2d', 4, 48, 48, 256, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 2, 3, 1),
    ('layout', ('2d', 4, 12, 12, 2048, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 5, 24, 24, 256, 256, 3, False, 1, 1, False, False)): (3, 3, 3, 2, 3, 1),
    ('layout', ('2d', 5, 48, 48, 256, 256, 3, False, 1, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 5, 24, 24, 256, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 2, 3, 1),
    ('layout', ('2d', 5, 48, 48, 256, 256, 4, True, 2, 1, False, False)): (2, 3, 3, 2, 3, 2),
    ('layout', ('2d', 5, 12, 12, 2048, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 19, 24, 24, 256, 256, 3, False, 1, 1, False, False)): (3, 3, 3, 2, 3, 1),
    ('layout', ('2d', 19, 48, 48, 256, 256, 3, False, 1, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 19, 24, 24, 256, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 2, 3, 1),
    ('layout', ('2d', 19, 48, 48, 256, 256, 4, True, 2, 1, False, False)): (2, 3, 3, 2, 3, 2),
    ('layout', ('2d', 19, 12, 12, 2048, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 20, 24, 24, 256, 256, 3, False, 1, 1, False, False)): (2, 3, 3, 2, 2, 2),
    ('layout', ('2d', 20, 48, 48, 256, 256, 3, False, 1, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 20, 24, 24, 256, 256, 4, True, 2, 1, False, False)): (2, 3, 3, 2, 3, 2),
    ('layout', ('2d', 20, 48, 48, 256, 256, 4, True, 2, 1, False, False)): (2, 3, 3, 2, 3, 2),
    ('layout', ('2d', 20, 12, 12, 2048, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 64, 24, 24, 256, 256, 3, False, 1, 1, False, False)): (2, 3, 3, 2, 2, 2),
    ('layout', ('2d', 64, 48, 48, 256, 256, 3, False, 1, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 64, 24, 24, 256, 256, 4, True, 2, 1, False, False)): (2, 3, 3, 2, 3, 2),
    ('layout', ('2d', 64, 48, 48, 256, 256, 4, True, 2, 1, False, False)): (2, 3, 3, 2, 3, 2),
    ('layout', ('2d', 64, 12, 12, 2048, 256, 4, True, 2, 1, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 5, 24, 24, 256, 256, 3, False, 1, 1, True, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 5, 24, 24, 256, 256, 3, False, 1, 1, False, True)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 5, 24, 24, 1024, 256, 1, False, 1, 0, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 5, 24, 24, 256, 1024, 1, False, 1, 0, False, False)): (1, 1, 1, 1, 1, 1),
    ('layout', ('2d', 5, 96, 96, 64, 256, 1, False, 1, 0, False, False)): (1, 1, 1, 1, 1, 1),
    ('layout', ('2d', 5, 96, 96, 64, 64, 3, False, 1, 1, False, False)): (0, 0, 0, 0, 0, 0),
    ('layout', ('2d', 5, 48, 48, 256, 512, 1, False, 2, 0, False, False)): (1, 1, 1, 1, 1, 1),
    ('layout', ('2d', 20, 24, 24, 256, 256, 3, False, 1, 1, True, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 20, 24, 24, 256, 256, 3, False, 1, 1, False, True)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 20, 24, 24, 1024, 256, 1, False, 1, 0, False, False)): (3, 3, 3, 3, 3, 1),
    ('layout', ('2d', 20, 24, 24, 256, 1024, 1, False, 1, 0, False, False)): (1, 1, 1, 1, 1, 1),
    ('layout', ('2d', 20, 96, 96, 64, 256, 1, False, 1, 0, False, False)): (1, 1, 1, 1, 1, 1),
    ('layout', ('2d', 20, 96, 96, 64, 64, 3, False, 1, 1, False, False)): (0, 0, 0, 0, 0, 0),
    ('layout', ('2d', 20, 48, 48, 256, 512, 1, False, 2, 0, False, False)): (1, 1, 1, 1, 1, 1),
    ('layout', ('3d', 1, 16, 16, 64, 64, 3, False, 1, 1, False, False)): (2, 2, 2, 2, 2, 2),
    ('layout', ('3d', 1, 16, 16, 32, 64, 3, False, 1, 1, False, False)): (2, 2, 2, 2, 2, 2),
    ('layout', ('3d', 1, 16, 16, 128, 128, 3, False, 1, 1, False, False)): (2, 2, 2, 2, 2, 2),
    ('layout', ('3d', 1, 16, 16, 16, 32, 3, False, 1, 1, False, False)): (2, 2, 2, 2, 2, 2),
    ('layout', ('3d', 1, 16, 16, 32, 32, 3, False, 1, 1, False, False)): (0, 0, 0, 0, 0, 0),
    ('layout', ('3d', 1, 16, 16, 64, 128, 3, False, 1, 1, False, False)): (0, 0, 0, 0, 0, 0),
    ('layout', ('3d', 1, 16, 16, 32, 64, 3, False, 2, 1, False, False)): (0, 0, 0, 0, 0, 0),
    ('layout', ('3d', 1, 16, 16, 64, 64, 2, True, 2, 0, False, False)): (0, 0, 0, 0, 0, 0),
    ('layout', ('3d', 4, 16, 16, 64, 64, 3, False, 1, 1, False, False)): (2, 2, 2, 2, 2, 2),
    ('layout', ('3d', 4, 16, 16, 32, 64, 3, False, 1, 1, False, False)): (2, 2, 2, 2, 2, 2),
    ('layout', ('3d', 4, 16, 16, 128, 128, 3, False, 1, 1, False, False)): (2, 2, 2, 2, 2, 2),
    ('layout', ('3d', 4, 16, 16, 16, 32, 3, False, 1, 1, False, False)): (2, 2, 2, 2, 2, 2),
    ('layout', ('3d', 4, 16, 16, 32, 32, 3, False, 1, 1, False, False)): (0, 0, 0, 0, 0, 0),
    ('layout', ('3d', 4, 16, 16, 64, 128, 3, False, 1, 1, False, False)): (0, 0, 0, 0, 0, 0),
    ('layout', ('3d', 4, 16, 16, 32, 64, 3, False, 2, 1, False, False)): (0, 0, 0, 0, 0, 0),
    ('layout', ('3d', 4, 16, 16, 64, 64, 2, True, 2, 0, False, False)): (0, 0, 0, 0, 0, 0),
}


def _layout(pb, spec, weight, transposed, residual):
    return pb.frag_layout(spec, weight, transposed, residual)


@pytest.fixture(scope="module")
def builders():
    return E.PlanBuilder("cpu", torch.bfloat16, dry_run=True), E.PlanBuilder("cpu", torch.float32, dry_run=True)


@pytest.mark.parametrize("rule,args", cases(), ids=lambda v: str(v).replace(" ", ""))
def test_selection_frozen(rule, args, builders, monkeypatch):
    pb, pb32 = builders
    for env in ENVS.values():
        for k in env:
            monkeypatch.delenv(k, raising=False)
    want = EXPECTED[(rule, args)]
    base = ev(pb, rule, args, _layout)
    got = [base]
    for k in ENVS[rule]:
        monkeypatch.setenv(k, "1")
        got.append(ev(pb, rule, args, _layout))
        for off in ("0", ""):
            monkeypatch.setenv(k, off)
            assert ev(pb, rule, args, _layout) == base, (k, off)
        monkeypatch.delenv(k)
    if rule != "layout":
        got.append(ev(pb32, rule, args, _layout))
    assert tuple(got) == want
