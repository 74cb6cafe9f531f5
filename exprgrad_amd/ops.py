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
