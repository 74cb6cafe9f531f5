"""Library fast path (group 2 of the C ABI) on raw device pointers.

Arguments are device addresses (ints): GpuBuffer.ptr, GpuTensor.ptr or torch.Tensor.data_ptr().
All calls enqueue on the context's stream and return immediately.
"""
import ctypes

from ._lib import call

MAP_OPS = {
    "identity": 0, "relu": 1, "leaky_relu": 2, "sigmoid": 3, "tanh": 4,
    "scale": 5, "sin": 6, "xor_leaky": 7, "exp": 8,
}


def _p(x):
    if x is None:
        return ctypes.c_void_p(0)
    if hasattr(x, "data_ptr"):
        x = x.data_ptr()
    elif hasattr(x, "ptr"):
        x = x.ptr
    return ctypes.c_void_p(int(x))


def sgemm(ctx, M, N, K, A, lda, B, ldb, C, ldc, trans_a=False, trans_b=False, accumulate=False, bias=None):
    call("eg_sgemm", ctx.handle, int(trans_a), int(trans_b), M, N, K, _p(A), lda, _p(B), ldb, _p(C), ldc,
         int(accumulate), _p(bias))


def sgemm_batched(ctx, batch, M, N, K, A, lda, stride_a, B, ldb, stride_b, C, ldc, stride_c, trans_a=False, trans_b=False,
                  accumulate=False, bias=None):
    """`batch` products of one shape in one launch: item b uses A + b * stride_a, B + b * stride_b, C + b * stride_c
    (strides in floats; stride_a / stride_b 0: the operand is shared).  Always the exact f32 path."""
    call("eg_sgemm_batched", ctx.handle, int(trans_a), int(trans_b), batch, M, N, K, _p(A), lda, stride_a, _p(B), ldb, stride_b,
         _p(C), ldc, stride_c, int(accumulate), _p(bias))


def sgemm_batched2(ctx, batch0, batch1, M, N, K, A, lda, strides_a, B, ldb, strides_b, C, ldc, strides_c, trans_a=False, trans_b=False,
                   accumulate=False, bias=None):
    """batch0 x batch1 products of one shape: item (o, i) uses X + o * strides_x[0] + i * strides_x[1] (pairs of strides in
    floats; a 0 in strides_a / strides_b shares the operand along that index; the items of C may interleave but not
    overlap).  Always the exact f32 path."""
    call("eg_sgemm_batched2", ctx.handle, int(trans_a), int(trans_b), batch0, batch1, M, N, K, _p(A), lda, strides_a[0], strides_a[1],
         _p(B), ldb, strides_b[0], strides_b[1], _p(C), ldc, strides_c[0], strides_c[1], int(accumulate), _p(bias))


def attention(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o,
              accumulate=False):
    """Fused attention forward, one launch: for every item (o, i1), O[i,:] (+)= (sum_j exp(scale * q_i . k_j) * V[j,:]) /
    (sum_j exp(scale * q_i . k_j)), as written, without the row maximum.  Item (o, i1) of X starts at X + o * strides_x[0] +
    i1 * strides_x[1] (floats; a 0 in the strides of Q, Kk or V shares the operand along that index).  K and D at most 128."""
    call("eg_attention", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], int(accumulate))


def attention_sums(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o, Sums,
                   strides_s, accumulate=False):
    """`attention` that also stores each row's denominator L_i = sum_j exp(scale * q_i . k_j), which attention_grad needs: item
    (o, i1) writes I floats at Sums + o * strides_s[0] + i1 * strides_s[1].  O has the bits `attention` gives; Sums is always
    overwritten (accumulate concerns O only); Sums = None is `attention`."""
    call("eg_attention_sums", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], int(accumulate), _p(Sums),
         strides_s[0], strides_s[1])


def attention_f64(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o,
                  accumulate=False):
    """The float64 form of `attention`: the same formula and addressing in doubles (leading dimensions and strides in doubles,
    the scale a double), on the float64 matrix instruction.  K and D at most 128."""
    call("eg_attention_f64", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], int(accumulate))


def attention_sums_f64(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o,
                       Sums, strides_s, accumulate=False):
    """The float64 form of `attention_sums`: item (o, i1) also writes its I denominators, doubles, at Sums + o * strides_s[0] +
    i1 * strides_s[1].  O has the bits `attention_f64` gives; Sums is always overwritten; Sums = None is `attention_f64`."""
    call("eg_attention_sums_f64", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], int(accumulate), _p(Sums),
         strides_s[0], strides_s[1])


def attention_grad(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o, Sums,
                   strides_s, dO, lddo, strides_do, dQ, lddq, strides_dq, dK, lddk, strides_dk, dV, lddv, strides_dv, accumulate=0):
    """Fused attention backward, two launches that store nothing of size I x J: from Q, Kk, V, the forward's O and Sums
    (attention_sums with accumulate = False) and dO, the gradients dQ [I, K], dK [J, K] and dV [J, D] of every item.  Strides as
    pairs of floats, as in `attention`; accumulate bit 0 adds to dQ, bit 1 to dK, bit 2 to dV.  K and D at most 128."""
    call("eg_attention_grad", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], _p(Sums), strides_s[0],
         strides_s[1], _p(dO), lddo, strides_do[0], strides_do[1], _p(dQ), lddq, strides_dq[0], strides_dq[1], _p(dK), lddk, strides_dk[0],
         strides_dk[1], _p(dV), lddv, strides_dv[0], strides_dv[1], int(accumulate))


def attention_bias(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o, Sums,
                   strides_s, Bias, ldb, strides_b, accumulate=False):
    """`attention_sums` with an additive score bias: e_ij = exp(scale * q_i . k_j + Bias[i * ldb + j]), item (o, i1) of Bias at
    Bias + o * strides_b[0] + i1 * strides_b[1].  Each of ldb and the two strides may be 0: the bias is then shared by the query
    rows (a key-padding mask), over batch0 or over batch1.  -Inf masks a key; Sums = None and Bias = None are allowed."""
    call("eg_attention_bias", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], int(accumulate), _p(Sums),
         strides_s[0], strides_s[1], _p(Bias), ldb, strides_b[0], strides_b[1])


def attention_bias_grad(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o, Sums,
                        strides_s, dO, lddo, strides_do, dQ, lddq, strides_dq, dK, lddk, strides_dk, dV, lddv, strides_dv, Bias, ldb, strides_b,
                        accumulate=0):
    """`attention_grad` for the biased forward: O and Sums from attention_bias (accumulate = False) on the same operands and the
    same Bias; p_ij = exp(scale * q_i . k_j + bias_ij) / L_i.  No gradient of the bias is produced.  Bias = None is
    `attention_grad`."""
    call("eg_attention_bias_grad", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], _p(Sums), strides_s[0],
         strides_s[1], _p(dO), lddo, strides_do[0], strides_do[1], _p(dQ), lddq, strides_dq[0], strides_dq[1], _p(dK), lddk, strides_dk[0],
         strides_dk[1], _p(dV), lddv, strides_dv[0], strides_dv[1], int(accumulate), _p(Bias), ldb, strides_b[0], strides_b[1])


def attention_bias_dbias(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o, Sums,
                         strides_s, dO, lddo, strides_do, Bias, ldb, strides_b, dBias, lddb, strides_db, accumulate=False):
    """The gradient of `attention_bias`'s Bias, one launch that stores nothing of size I x J but dBias itself: with O and Sums
    from attention_bias (accumulate = False) on the same operands and the same Bias, dBias (+)= the sum of p_ij * (dO_i . v_j -
    dO_i . o_i) over every index whose step in dBias is 0.  lddb and strides_db are 0 exactly where ldb and strides_b are: the
    gradient has the bias's broadcast form.  K and D at most 128."""
    call("eg_attention_bias_dbias", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], _p(Sums), strides_s[0],
         strides_s[1], _p(dO), lddo, strides_do[0], strides_do[1], _p(Bias), ldb, strides_b[0], strides_b[1], _p(dBias), lddb, strides_db[0],
         strides_db[1], int(accumulate))


def attention_stable(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o,
                     Stats=None, lds=0, strides_s=(0, 0), Bias=None, ldb=0, strides_b=(0, 0), accumulate=False):
    """Attention with a running row maximum: e_ij = exp(x_ij - max_j x_ij), x_ij = scale * q_i . k_j (+ Bias[i * ldb + j]), finite
    for finite scores of any magnitude where `attention` and `attention_bias` compute exp(x_ij) as written.  Item (o, i1) writes
    two rows of I floats at Stats + o * strides_s[0] + i1 * strides_s[1]: the maxima, and lds floats on the sums, which
    attention_stable_grad needs.  Stats = None and Bias = None are allowed; the bias has attention_bias's broadcast forms."""
    call("eg_attention_stable", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], int(accumulate), _p(Stats),
         lds, strides_s[0], strides_s[1], _p(Bias), ldb, strides_b[0], strides_b[1])


def attention_stable_split(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o,
                           Stats=None, lds=0, strides_s=(0, 0), Bias=None, ldb=0, strides_b=(0, 0), accumulate=False, splits=0):
    """`attention_stable` with every item's keys split into `splits` ranges of 64-key tiles (0: the library chooses; more than
    there are tiles: one per tile): one block per item, row tile and range, and one launch that combines them.  For few query
    rows against many keys, where `attention_stable` leaves most of the device idle; up to 16 rows the four waves of a block
    share the keys of a tile.  The same result to rounding, not to the bit; Stats serve attention_stable_grad."""
    call("eg_attention_stable_split", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], int(accumulate), _p(Stats),
         lds, strides_s[0], strides_s[1], _p(Bias), ldb, strides_b[0], strides_b[1], int(splits))


def attention_stable_grad(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o,
                          Stats, lds, strides_s, dO, lddo, strides_do, dQ, lddq, strides_dq, dK, lddk, strides_dk, dV, lddv, strides_dv,
                          Bias=None, ldb=0, strides_b=(0, 0), accumulate=0):
    """`attention_bias_grad` for the forward with a row maximum: O and Stats from attention_stable (accumulate = False) on the same
    operands and the same Bias; p_ij = exp(x_ij - max_i) / L_i.  accumulate bit 0 adds to dQ, bit 1 to dK, bit 2 to dV."""
    call("eg_attention_stable_grad", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], _p(Stats), lds,
         strides_s[0], strides_s[1], _p(dO), lddo, strides_do[0], strides_do[1], _p(dQ), lddq, strides_dq[0], strides_dq[1], _p(dK), lddk,
         strides_dk[0], strides_dk[1], _p(dV), lddv, strides_dv[0], strides_dv[1], int(accumulate), _p(Bias), ldb, strides_b[0], strides_b[1])


def attention_causal(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o,
                     Stats=None, lds=0, strides_s=(0, 0), Bias=None, ldb=0, strides_b=(0, 0), accumulate=False, offset=0):
    """`attention_stable` under a causal mask: key j is visible to query row i iff j <= i + offset (0: the diagonal of
    self-attention; J - I: a step against a key/value cache; negative: refused).  Key tiles without a visible key are never
    loaded or computed; O and Stats have the bits of `attention_stable` with a Bias of -inf at the masked pairs."""
    call("eg_attention_causal", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], int(accumulate), _p(Stats),
         lds, strides_s[0], strides_s[1], _p(Bias), ldb, strides_b[0], strides_b[1], int(offset))


def attention_causal_split(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o,
                           Stats=None, lds=0, strides_s=(0, 0), Bias=None, ldb=0, strides_b=(0, 0), accumulate=False, offset=0, chunk=0):
    """`attention_causal` with every 64-row tile's visible key tiles cut into pieces of at most `chunk` tiles (0: the library
    chooses), one block per piece, and one launch that combines the rows of the cut row tiles.  For a chunk of query rows or a
    decode step against a long key/value cache, or one long sequence; Stats serve `attention_causal_grad`."""
    call("eg_attention_causal_split", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], int(accumulate), _p(Stats),
         lds, strides_s[0], strides_s[1], _p(Bias), ldb, strides_b[0], strides_b[1], int(offset), int(chunk))


def attention_causal_grad(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o,
                          Stats, lds, strides_s, dO, lddo, strides_do, dQ, lddq, strides_dq, dK, lddk, strides_dk, dV, lddv, strides_dv,
                          Bias=None, ldb=0, strides_b=(0, 0), accumulate=0, offset=0):
    """`attention_stable_grad` for `attention_causal`: O and Stats from it (accumulate = False) on the same operands, the same Bias
    and the same offset.  accumulate bit 0 adds to dQ, bit 1 to dK, bit 2 to dV."""
    call("eg_attention_causal_grad", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], _p(Stats), lds,
         strides_s[0], strides_s[1], _p(dO), lddo, strides_do[0], strides_do[1], _p(dQ), lddq, strides_dq[0], strides_dq[1], _p(dK), lddk,
         strides_dk[0], strides_dk[1], _p(dV), lddv, strides_dv[0], strides_dv[1], int(accumulate), _p(Bias), ldb, strides_b[0], strides_b[1],
         int(offset))


def attention_grad_f64(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, strides_q, Kk, ldk, strides_k, V, ldv, strides_v, O, ldo, strides_o, Sums,
                       strides_s, dO, lddo, strides_do, dQ, lddq, strides_dq, dK, lddk, strides_dk, dV, lddv, strides_dv, accumulate=0):
    """The float64 form of `attention_grad`: O and Sums from attention_sums_f64 (accumulate = False), every operand in doubles
    (leading dimensions and strides in doubles, the scale a double); accumulate bit 0 adds to dQ, bit 1 to dK, bit 2 to dV."""
    call("eg_attention_grad_f64", ctx.handle, batch0, batch1, I, J, K, D, float(scale), _p(Q), ldq, strides_q[0], strides_q[1], _p(Kk), ldk,
         strides_k[0], strides_k[1], _p(V), ldv, strides_v[0], strides_v[1], _p(O), ldo, strides_o[0], strides_o[1], _p(Sums), strides_s[0],
         strides_s[1], _p(dO), lddo, strides_do[0], strides_do[1], _p(dQ), lddq, strides_dq[0], strides_dq[1], _p(dK), lddk, strides_dk[0],
         strides_dk[1], _p(dV), lddv, strides_dv[0], strides_dv[1], int(accumulate))


def dgemm_batched(ctx, batch, M, N, K, A, lda, stride_a, B, ldb, stride_b, C, ldc, stride_c, trans_a=False, trans_b=False,
                  accumulate=False, bias=None):
    """The float64 form of sgemm_batched: item b uses A + b * stride_a, B + b * stride_b, C + b * stride_c (strides and
    leading dimensions in doubles; stride_a / stride_b 0: the operand is shared)."""
    call("eg_dgemm_batched", ctx.handle, int(trans_a), int(trans_b), batch, M, N, K, _p(A), lda, stride_a, _p(B), ldb, stride_b,
         _p(C), ldc, stride_c, int(accumulate), _p(bias))


def dgemm_batched2(ctx, batch0, batch1, M, N, K, A, lda, strides_a, B, ldb, strides_b, C, ldc, strides_c, trans_a=False, trans_b=False,
                   accumulate=False, bias=None):
    """The float64 form of sgemm_batched2: item (o, i) uses X + o * strides_x[0] + i * strides_x[1] (pairs of strides, and
    leading dimensions, in doubles; a 0 in strides_a / strides_b shares the operand along that index; the items of C may
    interleave but not overlap)."""
    call("eg_dgemm_batched2", ctx.handle, int(trans_a), int(trans_b), batch0, batch1, M, N, K, _p(A), lda, strides_a[0], strides_a[1],
         _p(B), ldb, strides_b[0], strides_b[1], _p(C), ldc, strides_c[0], strides_c[1], int(accumulate), _p(bias))


def bias_add(ctx, rows, cols, bias, out, accumulate=True):
    call("eg_bias_add", ctx.handle, rows, cols, _p(bias), _p(out), int(accumulate))


def colsum(ctx, rows, cols, x, out, accumulate=False):
    call("eg_colsum", ctx.handle, rows, cols, _p(x), _p(out), int(accumulate))


def rowsum(ctx, rows, cols, x, out, accumulate=False):
    call("eg_rowsum", ctx.handle, rows, cols, _p(x), _p(out), int(accumulate))


def total(ctx, n, x, out, accumulate=False):
    call("eg_sum", ctx.handle, n, _p(x), _p(out), int(accumulate))


def axpy(ctx, n, alpha, x, y):
    call("eg_axpy", ctx.handle, n, float(alpha), _p(x), _p(y))


def fill(ctx, n, value, out):
    call("eg_fill_f32", ctx.handle, n, float(value), _p(out))


def map_(ctx, op, n, x, out, param=0.0, accumulate=False):
    call("eg_map", ctx.handle, MAP_OPS[op], n, _p(x), _p(out), float(param), int(accumulate))


def map_grad(ctx, op, n, x, gout, gin, param=0.0, accumulate=False):
    call("eg_map_grad", ctx.handle, MAP_OPS[op], n, _p(x), _p(gout), _p(gin), float(param), int(accumulate))


def conv2_nhwc(ctx, N, H, W, C, F, FH, FW, img, flt, out, accumulate=False):
    call("eg_conv2_nhwc", ctx.handle, N, H, W, C, F, FH, FW, _p(img), _p(flt), _p(out), int(accumulate))


def conv2_nhwc_grad_filter(ctx, N, H, W, C, F, FH, FW, img, gout, gflt, accumulate=False):
    """gflt[f,dy,dx,c] (+)= sum gout[n,y,x,f] * img[n,y+dy,x+dx,c]  (derived from dnn.nim:45-49)."""
    call("eg_conv2_nhwc_grad_filter", ctx.handle, N, H, W, C, F, FH, FW, _p(img), _p(gout), _p(gflt), int(accumulate))


def conv2_nhwc_grad_image(ctx, N, H, W, C, F, FH, FW, flt, gout, gimg, accumulate=False):
    """gimg[n,y+dy,x+dx,c] (+)= sum gout[n,y,x,f] * flt[f,dy,dx,c]  (derived from dnn.nim:45-49)."""
    call("eg_conv2_nhwc_grad_image", ctx.handle, N, H, W, C, F, FH, FW, _p(flt), _p(gout), _p(gimg), int(accumulate))


def conv2_nhwc_f64(ctx, N, H, W, C, F, FH, FW, img, flt, out, accumulate=False):
    """conv2_nhwc over float64 tensors, any channel count."""
    call("eg_conv2_nhwc_f64", ctx.handle, N, H, W, C, F, FH, FW, _p(img), _p(flt), _p(out), int(accumulate))


def conv2_nhwc_grad_filter_f64(ctx, N, H, W, C, F, FH, FW, img, gout, gflt, accumulate=False):
    """conv2_nhwc_grad_filter over float64 tensors."""
    call("eg_conv2_nhwc_grad_filter_f64", ctx.handle, N, H, W, C, F, FH, FW, _p(img), _p(gout), _p(gflt), int(accumulate))


def conv2_nhwc_grad_image_f64(ctx, N, H, W, C, F, FH, FW, flt, gout, gimg, accumulate=False):
    """conv2_nhwc_grad_image over float64 tensors."""
    call("eg_conv2_nhwc_grad_image_f64", ctx.handle, N, H, W, C, F, FH, FW, _p(flt), _p(gout), _p(gimg), int(accumulate))
