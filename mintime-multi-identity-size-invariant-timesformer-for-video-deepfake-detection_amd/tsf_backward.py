"""Reverse launch sequence of the Size-Invariant TimeSformer (analytic backward, not torch autograd over torch ops).

Walks the layers last-to-first on the saved buffers of tsf_engine.tsf_forward:
    dgemm (NT over the forward's transposed weights, else NN) for activations, wgrad (TN, split-K + fp32 atomics) for weights,
    column sums for biases, the attention-core / LayerNorm / embedding / head adjoint kernels of csrc/tsf_bwd.hip.
`dx` is the running gradient of the residual stream and is updated in place.
"""
import os

import torch

from . import arch
from . import lib as L


def tsf_backward(model, feat, aux, params, dims, saved, dlogits, need_dfeat, need_dparams):
    dev = feat.device
    B, F, n = dims
    D, H, dh, C_in = model.dim, model.heads, model.dim_head, model.channels
    inner = H * dh
    N = 1 + F * n
    M = B * N
    eps = arch.LN_EPS
    scale = float(dh) ** -0.5
    grads, flat_grads = L.zero_grads(list(params), with_flat=True)
    P = list(params)
    idx = len(P)

    def take(k):
        nonlocal idx
        idx -= k
        return idx

    side = L.SideStream(dev)
    wT = saved.get("wT")                              # transposed weights (tsf_engine.tsf_forward): data gradients in NT form
    if wT is not None and getattr(model, "_wT_cache", {}).get("serial") != saved.get("wT_serial"):
        wT = None                                     # a later forward rewrote the persistent buffers (two graphs alive): the weights
                                                      # as stored are still this graph's (torch's version counters guard THEM): NN form
    if wT is not None:
        side.wait(saved["wT_ready"])

    def colsum(A, lda, rows, cols, out, amap=(0, 0, 0)):
        L.mt.colsum(A, lda, L.RowMap(*amap), rows, cols, out)

    def dgrad(dY, Wm, off, out, N_, K_):
        """out[M, N_] = dY[M, K_] . Wm[K_, N_]: NT over the transposed weight (wT[(li, off)] = Wm^T [N_, K_]) if there is one, else NN."""
        if wT is not None:
            L.gemm(L.OP_NT, dY, wT[(li, off)], out, M, N_, K_, K_, K_, N_)
        else:
            L.gemm(L.OP_NN, dY, Wm, out, M, N_, K_, K_, N_, N_)

    def wgrad(A, Bm, out, M_, N_, K_, lda, ldb, ldc, bias_out=None, **kw):
        """dW (+ db) on the side stream: reads A [K_,M_] and Bm [K_,N_], accumulates into zero-filled grads."""
        def run():
            L.gemm(L.OP_TN, A, Bm, out, M_, N_, K_, lda, ldb, ldc, epilogue=L.EPI_ATOMIC, split_k=0, **kw)
            if bias_out is not None:
                colsum(A, lda, K_, M_, bias_out, kw.get("a_map", (0, 0, 0)))
        return side.launch(run, reads=(A, Bm))

    def ln_bwd(dxn_, r_, g_, dx_cur, i_g, tgt, skip):
        """dx = LN'(dxn) + dx_cur (+ gamma / beta gradients, + column sums for the bias below).  In place, or -- when weight
        gradients that read dx_cur are still to come -- into a fresh buffer.  With the weight-gradient stream on, only dx is
        computed on the main stream (mt_layernorm_bwd_rows: 48 VGPRs, no LDS -- it co-resides with the weight-gradient GEMMs
        instead of waiting for their blocks to end); the three column sums are parameter gradients and go to the side stream."""
        if ln_oop:
            dx_new = torch.empty_like(dx_cur)
            x_, st_ = r_["x"], r_["stats"]
            L.mt.layernorm_bwd_rows(dxn_, x_, st_, g_, dx_new, dx_cur, M, D, None)
            side.launch(lambda: L.mt.layernorm_bwd_cols(dxn_, x_, st_, dx_new, grads[i_g], grads[i_g + 1], tgt, skip, M, D),
                        reads=(dxn_, x_, st_, dx_new))
            return dx_new
        L.mt.layernorm_bwd(dxn_, r_["x"], r_["stats"], g_, dx_cur, grads[i_g], grads[i_g + 1], M, D, 1, tgt, skip, None)
        return dx_cur

    # ---- head
    i0 = take(4)
    g, b_, w_h, b_h = P[i0:i0 + 4]
    pruned = bool(saved.get("pruned_last"))           # tsf_engine: the last layer ran its tail on the cls rows only
    Nh = 1 if pruned else N
    dx = torch.zeros(B, Nh, D, dtype=torch.float32, device=dev)
    L.mt.head_bwd(dlogits, saved["x_final"], g, b_, w_h, dx, grads[i0], grads[i0 + 1], grads[i0 + 2], grads[i0 + 3], B, Nh, D,
                  model.num_classes, eps)
    dx2 = dx.view(B * Nh, D)
    # Bias gradients of the Linears whose output gradient is the residual stream's (net.3 / to_out.0 / patch embedding) are the
    # column sums of dx2 at that point.  The first one (last layer's net.3.bias) takes a column-sum launch over the head's dx;
    # every later one is emitted by the LayerNorm backward that produced that dx2 (dx_colsum), so no pass re-reads dx2 for it.
    dxn = torch.empty(M, D, dtype=torch.float32, device=dev)
    du = torch.empty(M, 8 * D, dtype=torch.float32, device=dev)
    do = torch.empty(M, inner, dtype=torch.float32, device=dev)
    dqkv = torch.empty(M, 3 * inner, dtype=torch.float32, device=dev)
    # Joins with the weight-gradient stream.  The first version joined the two streams at every sub-block start (its du / dqkv
    # buffers are reused) and waited for the sub-block's first weight gradient before the LayerNorm backward overwrote dx2 in
    # place (MT_TSF_JOIN=1 restores that).  Every cross-queue wait costs the main queue 13-19 us even when the event is long
    # complete (tools/lab/queue_sync_cost.py), and a join stalls it until the side stream has caught up: 54 of them per step.
    # Now each sub-block writes du / dqkv / dx2 into FRESH buffers (the side launches that read the old ones pin them with
    # record_stream), so the main stream waits for nothing inside the layer loop.
    # With the side stream off every side.launch runs inline and every side.wait returns at once.
    join_each = os.environ.get("MT_TSF_JOIN", "0") == "1"
    ln_oop = side.enabled and not join_each           # fresh du / dqkv / dxn / dx2 per sub-block (dxn is read on the side stream too)

    for li in reversed(range(model.depth)):
        rec = saved["layers"][li]
        if pruned and li == model.depth - 1:
            # ---- last layer, dead rows pruned: feed-forward and the space attention's tail on the B cls rows (dx2 is [B, D])
            i0 = take(6)
            g, b_, w1, b1, w2, b2 = P[i0:i0 + 6]
            r = rec[2]
            du_c = torch.empty(B, 8 * D, dtype=torch.float32, device=dev)
            dxn_c = torch.empty(B, D, dtype=torch.float32, device=dev)
            wgrad(dx2, r["h"], grads[i0 + 4], D, 4 * D, B, D, 4 * D, 4 * D, bias_out=grads[i0 + 5])
            L.gemm(L.OP_NN, dx2, w2, du_c, B, 4 * D, D, D, 4 * D, 8 * D, epilogue=L.EPI_GEGLU_BWD, C2=r["u"], ldc2=8 * D, n_half=4 * D,
                   col_sum=grads[i0 + 3])
            wgrad(du_c, r["xn"], grads[i0 + 2], 8 * D, D, B, 8 * D, D, D)
            L.gemm(L.OP_NN, du_c, w1, dxn_c, B, D, 8 * D, 8 * D, D, D)
            side.wait()
            L.mt.layernorm_bwd(dxn_c, r["x"], r["stats"], g, dx2, grads[i0], grads[i0 + 1], B, D, 1, grads[i0 - 1], 0, None)
            r.clear()
            # space attention: out-projection on the cls rows (row stride N), the cls query's adjoint, then the full QKV tail
            i0 = take(5)
            g, b_, w_qkv, w_o, b_o = P[i0:i0 + 5]
            r = rec[1]
            wgrad(dx2, r["o"], grads[i0 + 3], D, inner, B, D, N * inner, inner)             # o's cls rows: ldb = N * inner
            L.gemm(L.OP_NN, dx2, w_o, do, B, inner, D, D, inner, N * inner)                 # row 0 of each clip's do; the rest is not read
            dqkv.zero_()                                                                    # the patch queries' gradients are zero
            L.mt.attn_bwd(r["qkv"], do, dqkv, aux.mask, aux.ident, B, H, F, n, 2, scale, None)
            wgrad(dqkv, r["xn"], grads[i0 + 2], 3 * inner, D, M, 3 * inner, D, D)
            dgrad(dqkv, w_qkv, 7, dxn, D, 3 * inner)
            dx_full = torch.zeros(B, N, D, dtype=torch.float32, device=dev)
            dx_full[:, 0, :] = dx2                                                          # the residual path: cls rows only
            dx2 = dx_full.view(M, D)
            dx2 = ln_bwd(dxn, r, g, dx2, i0, grads[i0 - 1], 0)
            r.clear()
            # time attention: unchanged
            i0 = take(5)
            g, b_, w_qkv, w_o, b_o = P[i0:i0 + 5]
            r = rec[0]
            side.wait()
            e_dx = wgrad(dx2, r["o"], grads[i0 + 3], D, inner, M, D, inner, inner)
            dgrad(dx2, w_o, 3, do, inner, D)
            L.mt.attn_bwd(r["qkv"], do, dqkv, aux.mask, aux.ident, B, H, F, n, 0, scale, None)
            wgrad(dqkv, r["xn"], grads[i0 + 2], 3 * inner, D, M, 3 * inner, D, D)
            dgrad(dqkv, w_qkv, 2, dxn, D, 3 * inner)
            if join_each:
                side.wait(e_dx)
            tgt, skip = (grads[1], N) if li == 0 else (grads[i0 - 1], 0)
            dx2 = ln_bwd(dxn, r, g, dx2, i0, tgt, skip)
            r.clear()
            continue
        # ---- feed-forward: x_out = h W2^T + b2 + x ; h = a*gelu(g) ; [a|g] = LN(x) W1^T + b1
        i0 = take(6)
        g, b_, w1, b1, w2, b2 = P[i0:i0 + 6]
        r = rec[2]
        if join_each:
            side.wait()                               # du / dx2 readers of the previous sub-block are done
        if ln_oop:
            du = torch.empty(M, 8 * D, dtype=torch.float32, device=dev)       # the previous one may still be read by a weight gradient
            dxn = torch.empty(M, D, dtype=torch.float32, device=dev)
        e_dx = wgrad(dx2, r["h"], grads[i0 + 4], D, 4 * D, M, D, 4 * D, 4 * D,
                     bias_out=grads[i0 + 5] if li == model.depth - 1 else None)
        if wT is not None:
            L.gemm(L.OP_NT, dx2, wT[(li, 14)], du, M, 4 * D, D, D, D, 8 * D, epilogue=L.EPI_GEGLU_BWD, C2=r["u"], ldc2=8 * D,
                   n_half=4 * D, col_sum=grads[i0 + 3])
        else:
            L.gemm(L.OP_NN, dx2, w2, du, M, 4 * D, D, D, 4 * D, 8 * D, epilogue=L.EPI_GEGLU_BWD, C2=r["u"], ldc2=8 * D, n_half=4 * D,
                   col_sum=grads[i0 + 3])             # net.0.bias gradient = column sums of du, taken in the epilogue
        wgrad(du, r["xn"], grads[i0 + 2], 8 * D, D, M, 8 * D, D, D)
        dgrad(du, w1, 12, dxn, D, 8 * D)
        if join_each:
            side.wait(e_dx)                           # LayerNorm backward updates dx2 in place
        dx2 = ln_bwd(dxn, r, g, dx2, i0, grads[i0 - 1], 0)                     # column sums -> space to_out.0.bias
        r.clear()
        # ---- attention blocks: x_out = o Wo^T + bo + x ; o = attn(qkv) ; qkv = LN(x) Wqkv^T
        for mode in (1, 0):
            i0 = take(5)
            g, b_, w_qkv, w_o, b_o = P[i0:i0 + 5]
            r = rec[mode]
            if join_each:
                side.wait()                           # dqkv / dx2 readers of the previous sub-block are done
            if ln_oop:
                dqkv = torch.empty(M, 3 * inner, dtype=torch.float32, device=dev)    # (the old one is pinned by the launch reading it)
                dxn = torch.empty(M, D, dtype=torch.float32, device=dev)
            e_dx = wgrad(dx2, r["o"], grads[i0 + 3], D, inner, M, D, inner, inner)
            dgrad(dx2, w_o, 8 if mode == 1 else 3, do, inner, D)
            L.mt.attn_bwd(r["qkv"], do, dqkv, aux.mask, aux.ident, B, H, F, n, mode, scale, None)
            wgrad(dqkv, r["xn"], grads[i0 + 2], 3 * inner, D, M, 3 * inner, D, D)
            dgrad(dqkv, w_qkv, 7 if mode == 1 else 2, dxn, D, 3 * inner)
            if join_each:
                side.wait(e_dx)
            # the updated dx2 feeds the sub-block below: time attention's to_out.0.bias (index i0 - 1), the previous layer's
            # net.3.bias (i0 - 1 as well: parameter order is ..., w2, b2 | g, b, w_qkv, w_o, b_o | ...), or -- below layer 0 --
            # the patch embedding's bias (index 1), which does not see the cls rows
            if mode == 0 and li == 0:
                tgt, skip = grads[1], N
            else:
                tgt, skip = grads[i0 - 1], 0
            dx2 = ln_bwd(dxn, r, g, dx2, i0, tgt, skip)
            r.clear()

    # ---- embeddings + patch embedding
    i0 = take(5)
    w_pe, b_pe, cls, pos_w, size_w = P[i0:i0 + 5]
    dx = dx2.view(B, N, D)
    L.mt.embed_bwd(dx, grads[i0 + 2], grads[i0 + 3], grads[i0 + 4], aux.positions, aux.sizes, B, F, n, D, pos_w.shape[0],
                   size_w.shape[0] if size_w is not None else 0)
    tok_map = (F * n, N, 1)      # token row r of the feature matrix lives at row (r/(F n))*N + 1 + r%(F n) of dx
    Mt = B * F * n
    side.wait()
    wgrad(dx2, feat, grads[i0], D, C_in, Mt, D, C_in, C_in, a_map=tok_map)     # (bias: emitted by the last LayerNorm backward)
    dfeat = None
    if need_dfeat:
        dfeat = torch.empty(Mt, C_in, dtype=torch.float32, device=dev)
        L.gemm(L.OP_NN, dx2, w_pe, dfeat, Mt, C_in, D, D, C_in, C_in, a_map=tok_map)
    side.wait()
    assert idx == 0
    L.grads_ready(model, params, flat_grads)
    out = []
    for gneed, gr in zip(need_dparams, grads):
        out.append(gr if gneed else None)
    return dfeat, out
