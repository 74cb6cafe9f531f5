"""The cases of the float64 convolution entry points (eg_conv2_nhwc_f64, eg_conv2_nhwc_grad_filter_f64,
eg_conv2_nhwc_grad_image_f64) and their host references, shared by tests/test_conv64_cases_cpu.py (which holds the
float64 references to the same sums in extended precision), tests/test_conv64_plan_cpu.py and tests/test_gpu_conv64.py.

Each case (N, H, W, C, F, FH, FW) is the smallest shape that reaches one way of going wrong in the implicit-GEMM kernel
(csrc/kernels/conv2_f64_mfma.hip); values are uniform in [-1, 1] from a fixed seed."""
import functools

import numpy as np

CASES = [
    (1, 9, 10, 17, 17, 3, 3),    # just past the band kernels' limits; odd C (8-byte loads); P = 56 < one tile; ragged M, N, K
    (2, 12, 11, 24, 40, 3, 3),   # K = 216 is no multiple of 16; F ragged
    (3, 20, 18, 32, 64, 3, 3),   # everything aligned; 13.5 pixel tiles: tiles straddle rows and images
    (1, 8, 40, 20, 33, 5, 2),    # FH != FW: the flip and the border are asymmetric
    (1, 5, 5, 18, 18, 5, 5),     # Ho = Wo = 1: the image gradient is all border
    (1, 6, 6, 4, 48, 3, 3),      # few channels, many filters: band and direct both decline
    (2, 7, 7, 64, 16, 1, 1),     # 1 x 1 filter: the eg_dgemm route
    (4, 34, 34, 32, 32, 3, 3),   # P = 4096: the filter gradient is sliced
]
SLICED_CASE = CASES[7]
BATCH_CASE = CASES[2]
ROLES = ("forward", "grad_filter", "grad_image")
LONGEST_CHAIN = 4096    # terms of the longest sum of any case (the filter gradient of SLICED_CASE)


def case_id(c):
    return "x".join(str(v) for v in c)


def shapes(c):
    N, H, W, C, F, FH, FW = c
    return {"img": (N, H, W, C), "flt": (F, FH, FW, C), "out": (N, H - FH + 1, W - FW + 1, F)}


@functools.lru_cache(maxsize=None)
def operands(c):
    """img, flt, gout of a case (float64, read-only)."""
    rng = np.random.default_rng(1000 + CASES.index(c) if c in CASES else sum(c))
    s = shapes(c)
    ops = {"img": rng.uniform(-1, 1, s["img"]), "flt": rng.uniform(-1, 1, s["flt"]), "gout": rng.uniform(-1, 1, s["out"])}
    for v in ops.values():
        v.setflags(write=False)
    return ops


def forward(img, flt, dtype=np.float64):
    """out[n,y,x,f] = sum_{dy,dx,c} img[n,y+dy,x+dx,c] * flt[f,dy,dx,c]: FH * FW matrix products."""
    img, flt = img.astype(dtype), flt.astype(dtype)
    F, FH, FW, C = flt.shape
    N, H, W, _ = img.shape
    Ho, Wo = H - FH + 1, W - FW + 1
    out = np.zeros((N, Ho, Wo, F), dtype)
    for dy in range(FH):
        for dx in range(FW):
            out += img[:, dy:dy + Ho, dx:dx + Wo, :] @ flt[:, dy, dx, :].T
    return out


def grad_filter(img, gout, FH, FW, dtype=np.float64):
    """gflt[f,dy,dx,c] = sum_{n,y,x} gout[n,y,x,f] * img[n,y+dy,x+dx,c]."""
    img, gout = img.astype(dtype), gout.astype(dtype)
    N, Ho, Wo, F = gout.shape
    C = img.shape[3]
    g = np.zeros((F, FH, FW, C), dtype)
    flat = gout.reshape(-1, F).T
    for dy in range(FH):
        for dx in range(FW):
            g[:, dy, dx, :] = flat @ np.ascontiguousarray(img[:, dy:dy + Ho, dx:dx + Wo, :]).reshape(-1, C)
    return g


def grad_image(flt, gout, H, W, dtype=np.float64):
    """gimg[n,y+dy,x+dx,c] = sum_{f} gout[n,y,x,f] * flt[f,dy,dx,c], summed over the (y, dy), (x, dx) that meet."""
    flt, gout = flt.astype(dtype), gout.astype(dtype)
    N, Ho, Wo, F = gout.shape
    _, FH, FW, C = flt.shape
    g = np.zeros((N, H, W, C), dtype)
    for dy in range(FH):
        for dx in range(FW):
            g[:, dy:dy + Ho, dx:dx + Wo, :] += gout @ flt[:, dy, dx, :]
    return g


@functools.lru_cache(maxsize=None)
def reference(c, role, dtype=np.float64):
    N, H, W, C, F, FH, FW = c
    o = operands(c)
    r = (forward(o["img"], o["flt"], dtype) if role == "forward" else
         grad_filter(o["img"], o["gout"], FH, FW, dtype) if role == "grad_filter" else grad_image(o["flt"], o["gout"], H, W, dtype))
    r.setflags(write=False)
    return r
