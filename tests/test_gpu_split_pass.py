"""The split pass of the split-bf16 product (kernels/gemm_split_pass.hip): an operand whose k runs along its leading
dimension is read in 16 k x 256 row tiles, 16 bytes per lane, and turned k-contiguous through LDS.  The planes it writes
and the elements it refuses are those of the unit path with 4-byte loads (EG_SPLIT_PASS_SCALAR=1), so C has the same
bits: in the four layouts, with tight and with padded leading dimensions (the padding full of NaN), with twice the rows
on the tiled operand; and one element that does not split, wherever it sits in a tile or in a block's run of tiles,
still hands the product to the exact kernel.  All at the smallest shape the gate admits, 4096 x 4096 x 2048."""
import hashlib

import numpy as np
import pytest

from exprgrad_amd import ops

pytestmark = pytest.mark.gpu

M, N, K = 4096, 4096, 2048
LAYOUTS = {"nn": (False, False), "nt": (False, True), "tn": (True, False), "tt": (True, True)}

_values = {}


def _matrix(which, rows, cols, ld):
    """rows x cols of U[-0.5, 0.5) (the same numbers for every layout and leading dimension) in a rows x ld array whose
    padding is NaN."""
    key = (which, rows * cols)
    if key not in _values:
        rng = np.random.default_rng(41 + len(key[0]) + ord(which[0]))
        _values[key] = (rng.random(rows * cols, dtype=np.float32) - 0.5).astype(np.float32)
    out = np.full((rows, ld), np.nan, dtype=np.float32)
    out[:, :cols] = _values[key].reshape(rows, cols)
    return out


def _operands(mode, n=N, pad_a=0, pad_b=0):
    ta, tb = LAYOUTS[mode]
    ra, ca = (K, M) if ta else (M, K)
    rb, cb = (n, K) if tb else (K, n)
    return _matrix("a", ra, ca, ca + pad_a), _matrix("b", rb, cb, cb + pad_b)


def _dev(ctx, arr):
    t = ctx.allocTensor(arr.shape)
    t.write(arr)
    return t


def _set(monkeypatch, name, on):
    if on:
        monkeypatch.setenv(name, "1")
    else:
        monkeypatch.delenv(name, raising=False)


def _product(ctx, monkeypatch, mode, da, db, dc, n=N, route="tiles"):
    """route: tiles (the default build), scalar (EG_SPLIT_PASS_SCALAR=1), exact (EG_NO_SPLIT_GEMM=1)."""
    ta, tb = LAYOUTS[mode]
    _set(monkeypatch, "EG_SPLIT_PASS_SCALAR", route == "scalar")
    _set(monkeypatch, "EG_NO_SPLIT_GEMM", route == "exact")
    ops.sgemm(ctx, M, n, K, da, da.shape[1], db, db.shape[1], dc, n, trans_a=ta, trans_b=tb)
    return dc.read()


def _digest(c):
    return hashlib.sha256(np.ascontiguousarray(c).tobytes()).hexdigest()


@pytest.mark.parametrize("pads", [(0, 0), (4, 260)], ids=["tight", "lda+4_ldb+260"])
@pytest.mark.parametrize("mode", sorted(LAYOUTS))
def test_c_has_the_unit_paths_bits(gpu_ctx, monkeypatch, mode, pads):
    """With ldb = N + 260 the 1 KiB rows of a tile start 16 bytes off a 1 KiB boundary; the NaN between the rows must
    reach neither C nor the flag (a fallback would give the exact kernel's bits)."""
    a, b = _operands(mode, pad_a=pads[0], pad_b=pads[1])
    da, db, dc = _dev(gpu_ctx, a), _dev(gpu_ctx, b), gpu_ctx.allocTensor((M, N))
    tiles = _product(gpu_ctx, monkeypatch, mode, da, db, dc)
    scalar = _product(gpu_ctx, monkeypatch, mode, da, db, dc, route="scalar")
    exact = _product(gpu_ctx, monkeypatch, mode, da, db, dc, route="exact")
    print(mode, pads, _digest(tiles), _digest(scalar))
    assert np.isfinite(tiles).all()
    assert not np.array_equal(tiles, exact), "the split route did not run"
    assert _digest(tiles) == _digest(scalar)


def test_twice_the_rows_on_the_tiled_operand(gpu_ctx, monkeypatch):
    """4096 x 8192 x 2048, NN: N = 8192 rows of op(B), 32 tiles per k-tile."""
    n = 2 * N
    a, b = _operands("nn", n=n)
    da, db, dc = _dev(gpu_ctx, a), _dev(gpu_ctx, b), gpu_ctx.allocTensor((M, n))
    tiles = _product(gpu_ctx, monkeypatch, "nn", da, db, dc, n=n)
    scalar = _product(gpu_ctx, monkeypatch, "nn", da, db, dc, n=n, route="scalar")
    exact = _product(gpu_ctx, monkeypatch, "nn", da, db, dc, n=n, route="exact")
    assert not np.array_equal(tiles, exact), "the split route did not run"
    assert _digest(tiles) == _digest(scalar)


# (k, row) of the element in the tiled operand, which is stored [k][row] with 4096 rows: 16 tiles per k-tile, 2048 tiles,
# and with two blocks per CU on 256 CUs a block's run is four tiles (block 1: tiles 4 .. 7 of k-tile 0).
POSITIONS = {
    "first": (0, 0),
    "last": (K - 1, 4095),
    "last_k_of_the_first_tile": (15, 0),
    "first_row_of_the_last_tile_of_a_run": (0, 7 * 256),
    "row_255_mod_256": (777, 3 * 256 + 255),
}
# 2^-120 with a full significand: the first piece is normal, the pieces behind it are below 2^-126
BAD = {"nan": np.nan, "inf": np.inf, "subnormal": 1e-40, "2^-120": 2.0 ** -120 * 1.2345678}

_clean = {}


def _clean_case(ctx, monkeypatch, mode):
    """Per layout, once: the clean operands on the device, and C of the tile route and of the exact route."""
    if mode not in _clean:
        a, b = _operands(mode)
        da, db, dc = _dev(ctx, a), _dev(ctx, b), ctx.allocTensor((M, N))
        tiles = _product(ctx, monkeypatch, mode, da, db, dc)
        exact = _product(ctx, monkeypatch, mode, da, db, dc, route="exact")
        assert not np.array_equal(tiles, exact)
        _clean[mode] = (a, b, da, db, dc, _digest(tiles), _digest(exact))
    return _clean[mode]


@pytest.mark.parametrize("value", sorted(BAD))
@pytest.mark.parametrize("where", sorted(POSITIONS))
@pytest.mark.parametrize("mode", ["nn", "tt"])
def test_one_element_that_does_not_split_falls_back(gpu_ctx, monkeypatch, mode, where, value):
    """NN: the tiled operand is B; TT: it is A.  C equals EG_NO_SPLIT_GEMM=1's to the bit, and the next call with clean
    operands runs the split product again (the flag holds the earlier call's epoch, not this one's)."""
    a, b, da, db, dc, clean_tiles, clean_exact = _clean_case(gpu_ctx, monkeypatch, mode)
    k, r = POSITIONS[where]
    bad = (b if mode == "nn" else a).copy()
    bad[k, r] = np.float32(BAD[value])
    dbad = _dev(gpu_ctx, bad)
    xa, xb = (da, dbad) if mode == "nn" else (dbad, db)
    got = _product(gpu_ctx, monkeypatch, mode, xa, xb, dc)
    want = _product(gpu_ctx, monkeypatch, mode, xa, xb, dc, route="exact")
    assert np.array_equal(got, want, equal_nan=True)
    assert _digest(want) != clean_exact
    again = _product(gpu_ctx, monkeypatch, mode, da, db, dc)
    assert _digest(again) == clean_tiles
