"""The reference's other two model families over libpccx.so (inference forward passes):

  * PPPF_AE (PPPF_AE.py:114-150) = PointNet++ encoder built from PointnetSAModule
    (pointnet_sa_module.py:38-93: FPS from index 0, ball query, gather, Conv-BN-ReLU stack, max)
    + FoldingNet decoder (PPPF_AE.py:50-109)                          -- SURVEY 8a rows a18, a19
  * PointCloudAE of pppe_pcd_ae.py:843-877 (MSG + two SA levels with kNN grouping, global conv,
    quantize_st, PCN decoder)                                          -- SURVEY 8a row a21

Same constructor arguments and state_dict keys as the reference (torch modules are parameter
containers only).  Every layer is a HIP kernel behind the C ABI: selection ops from ops.py, the
Conv/Linear stacks with eval-mode BatchNorm folded into weight and bias at pack time.  Activations
are kept channels-last ((rows, C)), so the reference's permutes disappear; torch only concatenates
and reshapes buffers.

PPPF_AE is a tuned path: its Conv/Linear stacks run on operand planes (csrc/planes.hip) in
one of three arithmetics -- f16x2 or bf16x3 planes, or exact-fp32 rows -- each stack on its SOURCE rows
only, in one chain kernel where one fits.  The file states that machinery once: _PLANES (the entry points
of the two planes arithmetics), Stack (the packed layers and every operand derived from them) and
run_planes (the one stack runner).  The pppe PointCloudAE forward runs its stacks through the same runner in f16x2 (the centred kNN
grouping written straight as operand planes, PointCloudAE._forward_h2); in the f32 and bf16x3 modes it is layer by layer on fp32 rows
(pccx_linear / pccx_linear_b3).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from .ops import _stream, stage


def _arith(matmul=None):
    """The arithmetic asked for: a layer's own, else pccx.DEFAULT_MATMUL read at call time (tests and bench.py switch it between calls)."""
    from . import DEFAULT_MATMUL
    return matmul or DEFAULT_MATMUL


def _ptr(t):
    return t.data_ptr() if t is not None else None


# The two planes arithmetics (the host mirror of PgArith<P> in csrc/planes.hip): the size function and the entry points by role.  An
# f16x2 entry point takes its bf16x3 sibling's arguments plus scale arguments in front of `out`: _pcall() puts them there.
_PLANES = {
    "bf16x3": dict(floats="pccx_planes_floats", operand="pccx_group_planes", operand_centred="pccx_group_planes_centred", gemm="pccx_planes_gemm", gemm_gather="pccx_planes_gemm_gather",
                   chain4="pccx_planes_chain4", chain4_gather="pccx_planes_chain4_gather", rows_affine="pccx_rows_affine_planes"),
    "f16x2": dict(floats="pccx_planes_floats_h2", operand="pccx_group_planes_h2", operand_centred="pccx_group_planes_centred_h2", gemm="pccx_planes_gemm_h2", gemm_gather="pccx_planes_gemm_gather_h2",
                  chain4="pccx_planes_chain4_h2", chain4_gather="pccx_planes_chain4_gather_h2", rows_affine="pccx_rows_affine_planes_h2",
                  member_max="pccx_planes_gemm_h2_member_max", max_amax="pccx_planes_gemm_h2_max_amax"),
}


def _pcall(ar, role, args, scales, out):
    """The entry point of `role` in the arithmetic `ar`: (*args, *scales [f16x2 only], *out, stream)."""
    name = _PLANES[ar].get(role)
    if name is None:
        raise _lib.PccxError(f"families: no {role} entry point in the {ar} arithmetic")
    _lib.call(name, *args, *(scales if ar == "f16x2" else ()), *out, _stream())


def _planes_out(ar, M, N, epilogue, group, device):
    """What a planes kernel writes for M input rows: epilogue 0 -> the planes of the (M, N) output in `ar`, 1 -> fp32 rows (M, N),
    2 -> (M // group, N) maxima over `group` consecutive rows."""
    if epilogue == 0:
        return torch.empty(getattr(_lib.load(), _PLANES[ar]["floats"])(M, N), device=device, dtype=torch.float32)
    return torch.empty(M if epilogue == 1 else M // group, N, device=device, dtype=torch.float32)


# ---- f16x2 scales (csrc/planes.hip, "the same layers in the f16x2 arithmetic"; the rules of csrc/pack_h2.hip) -------------------------
def _pow2_floor(x):
    m, e = math.frexp(x)                                    # x = m 2^e, m in [0.5, 1)
    return math.ldexp(1.0, e - 1)


def h2_act_scale(bound):
    """the power of two sigma with bound * sigma <= 2^15 (half of fp16's largest number)"""
    return _pow2_floor(32768.0 / max(float(bound), 2.0 ** -40))


def h2_w_scale(W):
    """the largest power of two tau with max|W| tau <= 2^14: the lo piece of all but negligible weights stays a normal fp16 number"""
    m = float(np.abs(W).max()) if W.size else 0.0
    return _pow2_floor(16384.0 / m) if m > 0 else 1.0


def ibp_layer(W, b, lo, hi, relu):
    """Interval bounds of act(W x + b s) over x in [lo, hi] (per channel) and s in (0, 1] (the stack's dynamic normalisation multiplies
    the biases by a power of two s <= 1), in float64, inflated by 1e-3 for the fp32 evaluation of the kernels."""
    Wp, Wn = np.maximum(W, 0.0), np.minimum(W, 0.0)
    nhi = Wp @ hi + Wn @ lo + np.maximum(b, 0.0)
    nlo = Wp @ lo + Wn @ hi + np.minimum(b, 0.0)
    nhi, nlo = nhi + 1e-3 * np.abs(nhi) + 1e-30, nlo - 1e-3 * np.abs(nlo) - 1e-30
    if relu:
        nhi, nlo = np.maximum(nhi, 0.0), np.maximum(nlo, 0.0)
    return nlo, nhi


def h2_prepare_stack(stack, lo, hi):
    """Give every layer of a Conv/Linear stack its f16x2 operands for inputs within [lo, hi] per channel (the stack's NORMALISED input:
    magnitudes <= 1): sigma_l from the interval bound of the layer's input, tau_l from its weights, the two fp16 planes of tau W as
    the GEMM's weight stream, the bias as sigma tau b.  Returns the bounds of the stack's output (a Stack keeps them: they say it is
    prepared)."""
    lib = _lib.load()
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    for l in stack:
        sig = h2_act_scale(max(float(np.abs(lo).max()), float(np.abs(hi).max())))
        tau = h2_w_scale(l.W_host)
        wp2 = torch.empty(lib.pccx_packed_linear_h2_floats(l.N, l.K), device=l.wp.device, dtype=torch.float32)
        _lib.call("pccx_pack_linear_h2", l.wp.data_ptr(), l.N, l.K, float(tau), wp2.data_ptr(), _stream())
        ws2 = torch.empty(lib.pccx_planes_gemm_weight_floats_h2(l.N, l.K), device=l.wp.device, dtype=torch.float32)
        _lib.call("pccx_pack_planes_gemm_h2", wp2.data_ptr(), l.N, l.K, ws2.data_ptr(), _stream())
        l.h2 = dict(sig=sig, tau=tau, ws=ws2, b=(l.b * float(sig * tau)).contiguous())
        lo, hi = ibp_layer(l.W_host, l.b_host, lo, hi, l.relu)
    if isinstance(stack, Stack):
        stack.derived.pop(("chain4", "f16x2"), None)
        stack.derived["h2"] = (lo, hi)
    return lo, hi


class FoldedLinear:
    """Conv1x1 / Linear (+ eval BatchNorm) (+ ReLU) packed for pccx_linear.  matmul: "f32" (exact-fp32 MFMA) or "bf16x3" (fp32
    products from three bf16 pieces per operand, pccx_linear_b3); None = pccx.DEFAULT_MATMUL at call time (the bf16 planes are
    built on the device the first time they are needed)."""

    def __init__(self, weight, bias, relu, bn=None, device="cuda", matmul=None):
        W = weight.detach().to("cpu", torch.float32).reshape(weight.shape[0], -1).clone()
        b = bias.detach().to("cpu", torch.float32).clone() if bias is not None else torch.zeros(W.shape[0])
        if bn is not None:                                  # y = (z - mean) / sqrt(var + eps) * gamma + beta
            scale = bn.weight.detach().cpu() / torch.sqrt(bn.running_var.detach().cpu() + bn.eps)
            W = W * scale[:, None]
            b = (b - bn.running_mean.detach().cpu()) * scale + bn.bias.detach().cpu()
        self.N, self.K, self.relu = W.shape[0], W.shape[1], int(bool(relu))
        W = W.contiguous()
        self.W_host, self.b_host, self.h2 = W.numpy().astype(np.float64), b.numpy().astype(np.float64), None   # for the f16x2 bounds
        wp = torch.zeros(_lib.load().pccx_packed_linear_floats(self.N, self.K), dtype=torch.float32)
        _lib.call("pccx_pack_linear", W.data_ptr(), self.N, self.K, wp.data_ptr())
        self.wp, self.b = wp.to(device), b.contiguous().to(device)
        self.matmul, self.wp3, self.ws3 = matmul, None, None

    def mode(self):
        m = _arith(self.matmul)
        return "bf16x3" if m == "f16x2" else m              # pccx_linear has no f16x2 form (f16x2 is an arithmetic of planes stacks): bf16x3

    def planes_mode(self):
        """the arithmetic of the layer as part of a planes stack: "f16x2" when asked for (the stacks of PPPF_AE.forward), else mode()"""
        return _arith(self.matmul)

    def _planes3(self):
        if self.wp3 is None:
            self.wp3 = torch.empty(_lib.load().pccx_packed_linear_b3_floats(self.N, self.K), device=self.wp.device, dtype=torch.float32)
            _lib.call("pccx_pack_linear_b3", self.wp.data_ptr(), self.N, self.K, self.wp3.data_ptr(), _stream())
        return self.wp3

    def _stream3(self):
        if self.ws3 is None:
            self.ws3 = torch.empty(_lib.load().pccx_planes_gemm_weight_floats(self.N, self.K), device=self.wp.device, dtype=torch.float32)
            _lib.call("pccx_pack_planes_gemm", self._planes3().data_ptr(), self.N, self.K, self.ws3.data_ptr(), _stream())
        return self.ws3

    def planes(self, x, M, epilogue=0, group=0, idx=None, member=None, ar="bf16x3", sig_next=None, dyn=None, amax=None, max_amax=False):
        """The layer on an activation kept in planes (csrc/planes.hip): x = the planes of the (M, K) input in the arithmetic `ar`, or,
        with idx (B, Mq, ns) int64 (-1 -> row 0), the source rows (B, N, ldp) of padded_rows() that the kernel gathers itself.
        epilogue 0 -> planes of the (M, N) output, 1 -> fp32 rows (M, N), 2 -> (M // group, N) max over `group` consecutive rows; member
        (M bytes, epilogue 2, f16x2): the maxima run over the rows marked 1 only.
        f16x2 (h2_prepare_stack first): x holds sigma * input; epilogue 0 writes sig_next * output, 1 / 2 write un-scaled values (times
        dyn[1]); amax: 8 floats the row epilogue folds the largest |value| into -- and the max epilogue (epilogue 2 on planes) with
        max_amax, which goes through pccx_planes_gemm_h2_max_amax."""
        if ar == "f16x2":
            h = self.h2
            ws, b, sig_in = h["ws"], h["b"], [float(h["sig"])]
            scales = [(float(sig_next) if epilogue == 0 else 1.0) / (h["sig"] * h["tau"]), _ptr(dyn), _ptr(amax)]
        else:
            ws, b, sig_in, scales = self._stream3(), self.b, [], []
        out = _planes_out(ar, M, self.N, epilogue, group, x.device)
        layer, to = [ws.data_ptr(), b.data_ptr(), self.N, self.relu], [out.data_ptr(), self.N]
        if member is not None:
            _pcall(ar, "member_max", [x.data_ptr(), M, self.K] + layer + [group, member.data_ptr()], scales[:2], to)
        elif max_amax:
            if ar != "f16x2" or epilogue != 2 or idx is not None or amax is None:
                raise _lib.PccxError("FoldedLinear.planes: max_amax is the f16x2 max epilogue on planes, with amax")
            _pcall(ar, "max_amax", [x.data_ptr(), M, self.K] + layer + [group], scales, to)
        elif idx is not None:
            _pcall(ar, "gemm_gather", [x.data_ptr(), x.shape[2], idx.data_ptr(), idx.shape[1] * idx.shape[2], x.shape[1], M, self.K] + layer +
                   [epilogue, group], sig_in + scales, to)
        else:
            _pcall(ar, "gemm", [x.data_ptr(), M, self.K] + layer + [epilogue, group], scales, to)
        return out

    def __call__(self, x):
        """x (M,K) f32 contiguous on the GPU -> (M,N)."""
        M = x.shape[0]
        out = torch.empty(M, self.N, device=x.device, dtype=torch.float32)
        b3 = self.mode() == "bf16x3"
        _lib.call("pccx_linear_b3" if b3 else "pccx_linear", x.data_ptr(), M, self.K, x.stride(0), (self._planes3() if b3 else self.wp).data_ptr(),
                  self.b.data_ptr(), self.N, self.relu, out.data_ptr(), self.N, _stream())
        return out


class Stack:
    """The packed layers of one Conv/Linear stack and, in one dict, every operand derived from them, built the first time it is needed:
    the chain4 weight stream per arithmetic (with the f16x2 chain's five scales), the wide-chain stream, and the output bounds
    h2_prepare_stack leaves.  Indexing, len and iteration are the layer list's; a slice is a Stack of its own.  The owner drops the
    Stack (PPPF_AE._packed = None) and everything derived goes with it."""

    def __init__(self, layers):
        self.layers, self.derived = list(layers), {}

    def __len__(self):
        return len(self.layers)

    def __iter__(self):
        return iter(self.layers)

    def __getitem__(self, i):
        return Stack(self.layers[i]) if isinstance(i, slice) else self.layers[i]

    def rows(self, x):
        """layer by layer on fp32 rows x (M, K) (pccx_linear / pccx_linear_b3) -> (M, N_last)"""
        for layer in self.layers:
            x = layer(x)
        return x

    def chain4(self, ar):
        """the chain4 kernels' weight stream in `ar`, the f16x2 chain's five scales (None for bf16x3) and the (bias, width) arguments"""
        h2 = ar == "f16x2"
        if ("chain4", ar) not in self.derived:
            if h2:
                h = [l.h2 for l in self.layers]
                sc = np.array([h[0]["sig"]] + [h[i]["sig"] / (h[i - 1]["sig"] * h[i - 1]["tau"]) for i in (1, 2, 3)] +
                              [1.0 / (h[3]["sig"] * h[3]["tau"])], dtype=np.float32)
                self.derived["chain4", ar] = torch.cat([x["ws"] for x in h]), sc
            else:
                self.derived["chain4", ar] = torch.cat([l._stream3() for l in self.layers]), None
        ws, sc = self.derived["chain4", ar]
        a = []
        for l in self.layers:
            a += [(l.h2["b"] if h2 else l.b).data_ptr(), l.N]
        return ws, sc, a

    def wide3(self):
        """the weight stream of pccx_planes_chain_wide (the first three layers)"""
        if "wide3" not in self.derived:
            l0, l1, l2 = self.layers[:3]
            ws = torch.empty(_lib.load().pccx_planes_chain_wide_weight_floats(l0.K), device=l0.wp.device, dtype=torch.float32)
            _lib.call("pccx_pack_planes_chain_wide", l0._planes3().data_ptr(), l1._planes3().data_ptr(), l2._planes3().data_ptr(),
                      l0.K, l0.N, l1.N, l2.N, ws.data_ptr(), _stream())
            self.derived["wide3"] = ws
        return self.derived["wide3"]


def cat_rows(parts):
    """torch.cat(parts, dim=-1) flattened to rows, written into a buffer whose row stride is a multiple of 4 floats: the layer
    kernels then take their 16-byte vector loads whatever the channel count (3, 131, 259, 1026 ...).  Returns the (rows, C) view."""
    lead = parts[0].shape[:-1]
    rows = 1
    for d_ in lead:
        rows *= int(d_)
    C = sum(int(p.shape[-1]) for p in parts)
    buf = torch.empty(rows, (C + 3) // 4 * 4, device=parts[0].device, dtype=torch.float32)
    off = 0
    for p in parts:
        c = int(p.shape[-1])
        buf[:, off:off + c].copy_(p.reshape(rows, c))
        off += c
    return buf[:, :C]


def _rows2d(p):
    """(.., C) -> (2-D rows, C, row stride); rows that are 2-D already keep their row stride (cat_rows() pads it)"""
    if p is None:
        return None, 0, 0
    if p.dim() != 2:
        p = p.reshape(-1, p.shape[-1]).contiguous()
    return p, int(p.shape[1]), int(p.stride(0))


def group_planes(feats, xyz=None, idx=None, ar="bf16x3", sig=None, dyn=None):
    """[feats | xyz] rows as the operand planes of a stack's first layer, in the arithmetic `ar` (f16x2: times sig * dyn[0]).  Either
    part may be None.  With idx (B, M, ns) int64: index_points(feats, idx) ++ index_points(xyz, idx) (pointnet_sa_module.py:73-83; -1 ->
    row 0) of feats (B, N, C) channels-last and xyz (B, N, 3).  Without: every row as it stands, fp32 rows (M, K) (row stride >= K)
    or (B, N, C) tables (:83 features first, xyz last -- the concatenated rows never exist).  Returns (planes, rows)."""
    n_src = int((feats if feats is not None else xyz).shape[1]) if idx is not None else 1
    (f0, C0, ld0), (f1, C1, ld1) = _rows2d(feats), _rows2d(xyz)
    if idx is not None:
        idx = idx.contiguous()
        rows, per_batch = idx.numel(), idx.shape[1] * idx.shape[2]
    else:
        rows, per_batch = int((f0 if f0 is not None else f1).shape[0]), 1
    out = _planes_out(ar, rows, C0 + C1, 0, 0, (f0 if f0 is not None else f1).device)
    _pcall(ar, "operand", [_ptr(f0), C0, ld0, _ptr(f1), C1, ld1, _ptr(idx), rows, per_batch, n_src],
           [float(sig) if sig is not None else None, _ptr(dyn)], [out.data_ptr()])
    return out, rows


def group_planes_centred(offsets, feats=None, idx=None, ar="bf16x3", sig=None, dyn=None, amax=None):
    """The kNN grouping of pppe_pcd_ae.py:599-606 as the operand planes of a stack's first layer, in the arithmetic `ar` (f16x2: times
    sig * dyn[0]): offsets (B, S, K, 3) = the centred neighbours (knn_points(..., patch_scale=1.0).knn), feats (B, N, C) channels-last
    gathered through idx (B, S, K) int64, or None.  The planes hold [C features | 3 offsets] -- features FIRST, the layout of
    group_planes -- so the layer that reads them has the reference's weight columns rotated by three (centred_first_layer()).  amax:
    8 floats that receive the largest |offset|.  Returns (planes, rows)."""
    B, S, K = int(offsets.shape[0]), int(offsets.shape[1]), int(offsets.shape[2])
    rows = B * S * K
    offsets = offsets.contiguous()
    f, C, ld = _rows2d(feats)
    if f is not None:
        idx = idx.contiguous()
    out = _planes_out(ar, rows, C + 3, 0, 0, offsets.device)
    _pcall(ar, "operand_centred", [_ptr(f), C, ld, offsets.data_ptr(), _ptr(idx) if f is not None else None, rows, S * K,
                                   int(feats.shape[1]) if f is not None else 1, _ptr(amax)],
           [float(sig) if sig is not None else None, _ptr(dyn)], [out.data_ptr()])
    return out, rows


def centred_first_layer(conv, bn, device):
    """The first Conv-BN-ReLU of a pppe set-abstraction stack (input [3 offsets | C features], pppe_pcd_ae.py:606) packed for the
    features-first planes of group_planes_centred: the same weights, columns rotated to [C features | 3 offsets]."""
    w = conv.weight.detach().reshape(conv.weight.shape[0], -1)
    return FoldedLinear(torch.cat([w[:, 3:], w[:, :3]], dim=1), None, True, bn, device)


def chain4_fits(stack):
    """The width patterns pccx_planes_chain4 is built for (sa1 / sa2 of PPPF_AE.py:29-34), every layer with ReLU."""
    if len(stack) != 4 or not all(l.relu for l in stack) or any(stack[i + 1].K != stack[i].N for i in range(3)):
        return False
    n = [l.N for l in stack]
    return (n[0] <= 32 and 32 < n[1] <= 64 and 32 < n[2] <= 64 and 64 < n[3] <= 128) or \
           (all(96 < v <= 128 for v in n[:3]) and 128 < n[3] <= 256)


def padded_rows(feats, xyz):
    """[features, xyz] of every source point as fp32 rows zero padded to a multiple of 32 channels: what the gathering kernels read.
    Returns (src (B, N, ldp), C)."""
    parts = [p for p in (feats, xyz) if p is not None]
    C = sum(int(p.shape[-1]) for p in parts)
    B, n_src = int(parts[0].shape[0]), int(parts[0].shape[1])
    src = torch.zeros(B, n_src, (C + 31) // 32 * 32, device=parts[0].device, dtype=torch.float32)
    off = 0
    for p in parts:
        src[..., off:off + p.shape[-1]] = p
        off += int(p.shape[-1])
    return src, C


def wide3_fits(stack):
    """The first three layers fit pccx_planes_chain_wide (sa3 of PPPF_AE.py:32-34: widths 241..256, 241..256, 497..512, all ReLU, input
    of 8 or 9 blocks of 32 channels)."""
    if len(stack) < 3 or not all(l.relu for l in stack[:3]) or stack[1].K != stack[0].N or stack[2].K != stack[1].N:
        return False
    return 240 < stack[0].N <= 256 and 240 < stack[1].N <= 256 and 496 < stack[2].N <= 512 and (stack[0].K + 31) // 32 in (8, 9)


def wide3_planes(stack, src, idx, rows):
    """relu(L2(relu(L1(relu(L0(gathered rows)))))) as bf16x3 planes, one kernel (pccx_planes_chain_wide).  src (B, N, ldp) from
    padded_rows(), idx (B, M, ns) int64."""
    l0, l1, l2 = stack[0], stack[1], stack[2]
    ws = stack.wide3()
    out = _planes_out("bf16x3", rows, l2.N, 0, 0, src.device)
    _lib.call("pccx_planes_chain_wide", src.data_ptr(), src.shape[-1], idx.data_ptr(), idx.shape[1] * idx.shape[2], src.shape[1], rows, l0.K,
              ws.data_ptr(), l0.b.data_ptr(), l0.N, l1.b.data_ptr(), l1.N, l2.b.data_ptr(), l2.N, out.data_ptr(), _stream())
    return out


_EPILOGUE = {"planes": 0, "rows": 1, "max": 2, "member": 2}


def run_planes(stack, x, M, want="rows", group=0, idx=None, member=None, ar="bf16x3", dyn=None, amax=None):
    """A Conv/Linear Stack on M input rows through the planes kernels -- the one place that walks a stack's layers.
    x: the operand planes of the (M, K) input in the arithmetic `ar`; or a PaddedRows, which the first kernel gathers row by row (an
    identity index); or, with idx (B, Mq, ns) int64 (-1 -> row 0), the source rows (B, N, ldp) of padded_rows() -- the grouped tensor of
    pointnet_sa_module.py:73-83 never exists.
    want: "rows" -> fp32 rows (M, N_last); "max" -> (M // group, N_last), the maximum over `group` consecutive rows (:91; layer by layer
    also group 16, and in f16x2 on planes with amax the last layer is pccx_planes_gemm_h2_max_amax, which folds amax like the rows);
    "member" -> the same maximum over the rows marked 1 in `member` (M bytes; f16x2); "planes" -> the output as planes (bf16x3).
    ONE kernel where the stack fits pccx_planes_chain4 (rows / max); three wide layers in one kernel and the last by itself for a gathered
    bf16x3 input that fits pccx_planes_chain_wide; else layer by layer, the first layer gathering and the last one reducing.
    f16x2: dyn = the stack's dynamic input normalisation {s, 1 / s} on the device, amax = 8 floats that receive the largest |value| of
    the fp32 rows written (h2_prepare_stack first)."""
    h2 = ar == "f16x2"
    if h2 and "h2" not in stack.derived:
        raise _lib.PccxError("run_planes: h2_prepare_stack() has not run on this stack")
    if isinstance(x, PaddedRows):
        Bn, n_src = x.src.shape[0], x.src.shape[1]
        x, idx = x.src, identity_index(Bn, n_src, x.src.device).view(Bn, n_src, 1)
    if want in ("rows", "max") and chain4_fits(stack):
        g = group if want == "max" else 1
        ws, sc, a = stack.chain4(ar)
        out = _planes_out(ar, M, stack[3].N, 2, g, x.device)
        scales, to = [sc.ctypes.data, _ptr(dyn), _ptr(amax)] if h2 else [], [out.data_ptr(), stack[3].N]
        if idx is not None:
            _pcall(ar, "chain4_gather", [x.data_ptr(), x.shape[2], idx.data_ptr(), idx.shape[1] * idx.shape[2], x.shape[1], M, stack[0].K,
                                         ws.data_ptr(), *a, g], scales, to)
        else:
            _pcall(ar, "chain4", [x.data_ptr(), M, stack[0].K, ws.data_ptr(), *a, g], scales, to)
        return out
    first = 0
    if idx is not None and not h2 and len(stack) == 4 and wide3_fits(stack):
        x, idx, first = wide3_planes(stack, x, idx, M), None, 3
    for i, layer in enumerate(stack[first:-1], start=first):
        x, idx = layer.planes(x, M, 0, idx=idx, ar=ar, sig_next=stack[i + 1].h2["sig"] if h2 else None, dyn=dyn), None
    return stack[-1].planes(x, M, _EPILOGUE[want], group, idx=idx, member=member, ar=ar, dyn=dyn, amax=amax,
                            max_amax=h2 and want == "max" and idx is None and amax is not None)


def stack_max_gather(stack, feats, xyz, idx):
    """index_points(feats, idx) ++ index_points(xyz, idx) -> Conv-BN-ReLU stack -> max over nsample (pointnet_sa_module.py:73-91), bf16x3:
    the gather happens inside the first kernel from the (B, N, C+3) rows of padded_rows().  idx (B, M, ns) int64.  Returns (B * M, N_last)."""
    return run_planes(stack, padded_rows(feats, xyz)[0], idx.numel(), "max", idx.shape[2], idx=idx.contiguous())


def stack_max_planes(stack, pl, rows, group):
    """Conv-BN-ReLU stack + max over `group` consecutive rows on bf16x3 planes."""
    return run_planes(stack, pl, rows, "max", group)


def fold_planes(a, mod0, b, div1, M):
    """torch.cat([a rows, b rows repeated], -1) as planes without building it: row r = a[r % mod0 if mod0 else r] ++ b[r // div1]
    (PPPF_AE.py:99-106).  a (.., C0), b (.., C1) fp32 rows."""
    a, b = a.contiguous(), b.contiguous()
    C0, C1 = int(a.shape[-1]), int(b.shape[-1])
    out = _planes_out("bf16x3", M, C0 + C1, 0, 0, a.device)
    _lib.call("pccx_fold_planes", a.data_ptr(), C0, C0, mod0, b.data_ptr(), C1, C1, div1, M, out.data_ptr(), _stream())
    return out


def run_stack(stack, x):
    """A Conv/Linear Stack on fp32 rows x (M, K): layer by layer on rows (f32), or through planes (bf16x3)."""
    if len(stack) and stack[0].mode() == "bf16x3" and x.shape[0] > 0:
        return run_planes(stack, group_planes(x)[0], x.shape[0])
    return stack.rows(x)


def rows_affine_small(base, div, x, mod, w_small, relu, M, planes=None, rho=None, dyn=None):
    """act(base[r // div] + x[r % mod if mod else r] @ w_small.T) for r < M: base (B, C), x (.., Ks <= 4).  planes=None -> fp32 rows (M, C)
    (pccx_rows_affine_small); "bf16x3" / "f16x2" -> the same values written as the operand planes of the next layer, no fp32 rows in
    between (f16x2: times rho * dyn[0])."""
    x = x.contiguous()
    Cc, Ks = int(base.shape[-1]), int(w_small.shape[1])
    args = [base.contiguous().data_ptr(), Cc, int(div), x.data_ptr(), int(x.shape[-1]), Ks, int(mod), w_small.data_ptr(), int(bool(relu)), int(M)]
    if planes is None:
        out = torch.empty(M, Cc, device=base.device, dtype=torch.float32)
        _lib.call("pccx_rows_affine_small", *args, out.data_ptr(), _stream())
    else:
        out = _planes_out(planes, M, Cc, 0, 0, base.device)
        _pcall(planes, "rows_affine", args, [float(rho) if rho is not None else None, _ptr(dyn)], [out.data_ptr()])
    return out


def gather_max(y, idx):
    """max over nsample of y[b, idx.clamp(min=0)] (pointnet_sa_module.py:27-28,91): y (B,N,C) rows, idx (B,M,ns) int64 -> (B,M,C)."""
    B, N, Cc = y.shape
    _, M, ns = idx.shape
    out = torch.empty(B, M, Cc, device=y.device, dtype=torch.float32)
    _lib.call("pccx_gather_max", y.contiguous().data_ptr(), B, N, Cc, idx.contiguous().data_ptr(), M, ns, out.data_ptr(), _stream())
    return out


class PaddedRows:
    """The input rows of a set-abstraction level as the gathering planes kernels read them: src (B, N, ldp) fp32 with ldp = 32 * ceil((C + 3) / 32),
    row = [C features | xyz | zeros] (pointnet_sa_module.py:83: features first, xyz last)."""

    def __init__(self, src, C):
        self.src, self.C = src, int(C)


def gather_max_rows(y, idx, new_xyz):
    """gather_max whose output IS the next level's input rows (pccx_gather_max_rows): -> PaddedRows((B, M, ldp), C)"""
    B, N, Cc = y.shape
    _, M, ns = idx.shape
    ldp = (Cc + 3 + 31) // 32 * 32
    out = torch.empty(B, M, ldp, device=y.device, dtype=torch.float32)
    _lib.call("pccx_gather_max_rows", y.contiguous().data_ptr(), B, N, Cc, idx.contiguous().data_ptr(), M, ns, new_xyz.contiguous().data_ptr(),
              out.data_ptr(), ldp, _stream())
    return PaddedRows(out, Cc)


_IDENTITY = {}


def identity_index(P, n, device):
    """(P * n) int64: 0 .. n - 1 for each of the P batch elements (the gathering kernels' index of the rows as they stand)"""
    key = (int(P), int(n), str(device))
    t = _IDENTITY.get(key)
    if t is None:
        if len(_IDENTITY) > 8:
            _IDENTITY.clear()
        t = _IDENTITY[key] = torch.arange(n, device=device, dtype=torch.int64).repeat(P).contiguous()
    return t


def group_max(x):
    """(G,Kn,C) -> (G,C)."""
    G, Kn, Cc = x.shape
    out = torch.empty(G, Cc, device=x.device, dtype=torch.float32)
    _lib.call("pccx_group_max", x.contiguous().data_ptr(), G, Kn, Cc, out.data_ptr(), _stream())
    return out


def sigmoid_spread(x, L, do_round=False):
    y = torch.empty_like(x)
    _lib.call("pccx_sigmoid_spread", x.contiguous().data_ptr(), x.numel(), int(L), int(do_round), y.data_ptr(), _stream())
    return y


def round_(x):
    y = torch.empty_like(x)
    _lib.call("pccx_round", x.contiguous().data_ptr(), x.numel(), y.data_ptr(), _stream())
    return y


def _fold_stack(seq, device):
    """[Conv, (BN), (ReLU), ...] -> Stack of FoldedLinear."""
    mods = list(seq)
    out, i = [], 0
    while i < len(mods):
        conv = mods[i]
        i += 1
        bn = None
        if i < len(mods) and isinstance(mods[i], (nn.BatchNorm1d, nn.BatchNorm2d)):
            bn = mods[i]
            i += 1
        relu = i < len(mods) and isinstance(mods[i], nn.ReLU)
        if relu:
            i += 1
        out.append(FoldedLinear(conv.weight, conv.bias, relu, bn, device))
    return Stack(out)


class _Packable(nn.Module):
    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._packed = None
        return r


# =================================================================================================
# PPPF_AE
# =================================================================================================
class PointnetSAModule(nn.Module):                      # pointnet_sa_module.py:38-56
    def __init__(self, npoint, radius, nsample, mlp, use_xyz=True, in_channels=0):
        super().__init__()
        self.npoint, self.radius, self.nsample, self.use_xyz = npoint, radius, nsample, use_xyz
        last = in_channels + (3 if use_xyz else 0)
        layers = []
        for out in mlp:
            layers += [nn.Conv2d(last, out, 1), nn.BatchNorm2d(out), nn.ReLU(inplace=True)]
            last = out
        self.mlp = nn.Sequential(*layers)

    # The module gathers features and xyz UN-CENTRED (:73-85) and its Conv-BN(eval)-ReLU stack acts on each (group, sample) row by
    # itself, so every one of the npoint * nsample grouped rows is a copy of one of the N source rows: the stack is evaluated on
    # the N rows once and each group takes the maximum over its members from that result (pccx_gather_max) -- the same fp32 chain
    # per row, hence bit-identical outputs, for 1 / (npoint * nsample / N) of the matrix work (PPPF_AE: 16384 -> 512, 8192 -> 512,
    # 4096 -> 128 rows per patch).  dedup=False keeps the literal grouped evaluation (tests compare the two bit for bit).
    dedup = True
    # A level whose output is only ever reduced over ALL its centroids (PPPF_AE's third: PPPF_AE.py:44) needs no per-centroid maxima: the
    # maximum over the centroids of the maxima over their samples is the maximum over the source rows that are a sample of any centroid.
    # run(union=True) marks those rows (pccx_group_members) and takes that maximum in the last layer's epilogue -- neither the layer's
    # fp32 rows (1 GB per 2048 patches) nor the per-centroid table exist.  union_max=False keeps gather_max + group_max (tests compare).
    union_max = True
    # Between the f16x2 levels the maxima are written as the next level's padded input rows (pccx_gather_max_rows) and that level's first
    # kernel gathers them itself (the gathering forms of the chain / GEMM with an identity index): the operand-plane pass of levels 2 and 3
    # (0.23 + 0.11 ms per 2048 patches) is not run.  Same planes, same results; False keeps the plane pass (tests compare).
    padded_levels = True

    def run(self, stack, xyz, feats, dyn=None, amax=None, pad_out=False, union=False):
        """xyz (B,N,3); feats (B,N,C) channels-last or None -> (new_xyz (B,M,3), feats (B,M,C')).
        dyn: evaluate the stack in the f16x2 arithmetic (h2_prepare_stack has run): the level's dynamic input normalisation {s, 1 / s} on
        the device; amax = 8 floats that receive the largest value of the stack's output.  With dyn, feats may be a PaddedRows (the
        previous level's pad_out) and pad_out=True returns one: the maxima written as the NEXT level's input rows [features | new_xyz | 0],
        which its first kernel gathers itself -- no operand-plane pass between the levels.  union=True (f16x2, N in {32, 64, 128} source
        rows per element, last layer with ReLU): feats is (B, C'), the maximum over the npoint centroids of the level's output."""
        B, N = xyz.shape[0], xyz.shape[1]
        with stage("fps"):
            new_xyz, _ = ops.sample_farthest_points(xyz, self.npoint)               # :66-68 (start index 0)
        with stage("ball_query"):
            idx = ops.ball_query(new_xyz, xyz, self.nsample, self.radius).idx       # :71 (-1 padded; gather clamps, :27)
            member = torch.empty(B * N, device=xyz.device, dtype=torch.uint8) if union else None
            if union:
                _lib.call("pccx_group_members", idx.data_ptr(), idx.numel(), self.npoint * self.nsample, N, member.data_ptr(), _stream())
        if self.dedup and B > 0 and stack[-1].N % 4 == 0:
            return new_xyz, self._run_dedup(stack, xyz, feats, idx, dyn, amax, new_xyz if pad_out else None, member)
        if dyn is not None:
            raise _lib.PccxError("PointnetSAModule: the f16x2 stacks are built for the source-row evaluation (dedup=True)")
        return self._run_grouped(stack, xyz, feats, idx, new_xyz, B)

    def _run_dedup(self, stack, xyz, feats, idx, dyn=None, amax=None, pad_xyz=None, member=None):
        """the stack on the N SOURCE rows of every element, then each group's maximum over its members"""
        B, N = xyz.shape[0], xyz.shape[1]
        ar = "f16x2" if dyn is not None else stack[0].mode()
        with stage("sa_stack_%d" % stack[-1].N):
            if ar == "f32":
                y = stack.rows(cat_rows([feats, xyz] if feats is not None else [xyz]))      # :83 features first, xyz last; :90
            else:
                # rows -> planes of [features, xyz] (f16x2: times sigma_0 s) unless the previous level wrote them as PaddedRows, then ONE
                # chain kernel (sa1 / sa2) or the layers one by one (sa3); f16x2 un-scales and records the output's maximum in the last
                x = feats if isinstance(feats, PaddedRows) else \
                    group_planes(feats, xyz, ar=ar, sig=stack[0].h2["sig"] if dyn is not None else None, dyn=dyn)[0]
                if member is not None:
                    return run_planes(stack, x, B * N, "member", N, member=member, ar=ar, dyn=dyn)   # :44 and :91 in one epilogue
                y = run_planes(stack, x, B * N, ar=ar, dyn=dyn, amax=amax)                  # :90 Conv-BN-ReLU, (B * N, C) rows
        with stage("gather_max"):
            if pad_xyz is not None:
                return gather_max_rows(y.view(B, N, -1), idx, pad_xyz)                      # :91, written as the next level's input rows
            return gather_max(y.view(B, N, -1), idx)                                        # :91 max over the group's members

    def _run_grouped(self, stack, xyz, feats, idx, new_xyz, B):
        """the literal form: the stack on all npoint * nsample gathered rows (what dedup=False compares against)"""
        if stack[0].mode() == "bf16x3" and self.nsample in (32, 64, 128) and B > 0:
            # :73-91 gather (features first, xyz last, not centred) inside the first kernel, every layer on planes, max over nsample in the last
            return new_xyz, stack_max_gather(stack, feats, xyz, idx).view(B, self.npoint, -1)
        grouped = ops.index_points(xyz, idx)                                        # :81 (not centred)
        x = cat_rows([ops.index_points(feats, idx), grouped] if feats is not None else [grouped])   # :83 features first, xyz last
        x = stack.rows(x)                                                           # :90 Conv-BN-ReLU
        return new_xyz, group_max(x.view(B * self.npoint, self.nsample, -1)).view(B, self.npoint, -1)   # :91


class PointNetPP(nn.Module):                            # PPPF_AE.py:9-46
    def __init__(self, points=512, sa1_mlp=(64, 64, 128), sa2_mlp=(128, 128, 128, 256), sa3_mlp=(256, 256, 512),
                 feature_dim=1024):
        super().__init__()
        self.sa1 = PointnetSAModule(points, 0.2, 32, [3] + list(sa1_mlp), True, 0)
        self.sa2 = PointnetSAModule(128, 0.4, 64, list(sa2_mlp), True, 128)
        self.sa3 = PointnetSAModule(32, 0.8, 128, list(sa3_mlp) + [feature_dim], True, 256)


class FoldingNet(nn.Module):                            # PPPF_AE.py:50-80
    def __init__(self, points=512, grid_size=45, feature_dim=1024):
        super().__init__()
        self.grid_size, self.num_points = grid_size, grid_size * grid_size
        self.mlp1 = nn.Sequential(nn.Conv1d(feature_dim + 2, points, 1), nn.ReLU(), nn.Conv1d(points, points, 1), nn.ReLU(),
                                  nn.Conv1d(points, 3, 1))
        self.mlp2 = nn.Sequential(nn.Conv1d(feature_dim + 3, 128, 1), nn.ReLU(), nn.Conv1d(128, 128, 1), nn.ReLU(),
                                  nn.Conv1d(128, 3, 1))


class H2Scales:
    """The f16x2 scale bookkeeping of one packed model, rewritten by every forward on the device: amax = n_amax slots of 8 floats that
    receive a largest |value|, dyn = n_dyn slots {s, 1 / s}, one per planes stack: the power of two s <= 1 that normalises its input.
    PPPF_AE (the defaults): amax 0 coordinates, 1 / 2 outputs of levels 1 / 2, 3 / 5 per-patch parts of mlp1 / mlp2, 4 coarse points;
    dyn levels 0..2, mlp1, mlp2; wsum = the largest absolute row sums of the two folding MLPs' per-point weights.  PointCloudAE:
    PointCloudAE._SLOTS."""

    def __init__(self, device, wsum, n_amax=6, n_dyn=5):
        self.amax = torch.zeros(n_amax * 8, device=device, dtype=torch.float32)
        self.dyn = torch.ones(n_dyn * 2, device=device, dtype=torch.float32)
        self.wsum = wsum

    def __getitem__(self, name):                           # ._packed["h2"]["dyn"], as tests and bench.py read it
        return getattr(self, name)

    def am(self, i):
        return self.amax[8 * i:8 * i + 8] if i is not None else None

    def dy(self, i):
        return self.dyn[2 * i:2 * i + 2]

    def reset(self):
        _lib.call("pccx_zero_bytes", self.amax.data_ptr(), self.amax.numel() * 4, _stream())

    def absmax(self, t, i):
        """fold max |t| into amax slot i"""
        _lib.call("pccx_absmax", t.data_ptr(), t.numel(), self.am(i).data_ptr(), _stream())

    def scale(self, out, m1, m2=None, a2=0.0, add=0.0, comb=1):
        """dyn slot `out` from amax slot m1 and (comb 1: the larger of the two, comb 0: plus) a2 * amax slot m2 + add (pccx_dyn_scale)"""
        _lib.call("pccx_dyn_scale", self.am(m1).data_ptr(), 1.0, _ptr(self.am(m2)), float(a2), float(add), int(comb), self.dy(out).data_ptr(),
                  _stream())


def _pow2x4(n):
    """the widths pccx_rows_affine_small takes"""
    return n % 4 == 0 and n <= 1024 and (n // 4) & (n // 4 - 1) == 0


class PPPF_AE(_Packable):
    """PPPF_AE.PPPF_AE (PPPF_AE.py:114-150)."""

    split_fold = True       # FoldingNet's first layers evaluated as per-patch + per-point parts (_fold()); False = the literal rows
    # amax / dyn slots of the two folding MLPs in the f16x2 arithmetic: per-patch part, per-point input (None: the grid, within [-1, 1]),
    # the chain's normalisation, the chain's output
    _FOLD_SLOTS = {"mlp1": (3, None, 3, 4), "mlp2": (5, 4, 4, None)}

    def __init__(self, K=512, k=0, d=16, L=7, dim=1024):
        super().__init__()
        self.L, self.d, self.dim = L, d, dim
        self.encoder = PointNetPP(points=K, feature_dim=dim)
        self.decoder = FoldingNet(points=K, grid_size=d)
        self.enc_proj = nn.Linear(dim, d)
        self.dec_proj = nn.Linear(d, dim)
        self._packed = None

    def pack(self, device="cuda"):
        e, dcd = self.encoder, self.decoder
        self._packed = dict(sa=[_fold_stack(m.mlp, device) for m in (e.sa1, e.sa2, e.sa3)],
                            enc=FoldedLinear(self.enc_proj.weight, self.enc_proj.bias, False, None, device),
                            dec=FoldedLinear(self.dec_proj.weight, self.dec_proj.bias, False, None, device),
                            mlp1=_fold_stack(dcd.mlp1, device), mlp2=_fold_stack(dcd.mlp2, device))
        # first layers of the two folding MLPs split into their per-patch (latent) and per-point (grid / coarse) parts, see _fold();
        # _rest = the layers after the first, a Stack of its own
        for name, seq, ks in (("mlp1", dcd.mlp1, 2), ("mlp2", dcd.mlp2, 3)):
            w = seq[0].weight.detach().to("cpu", torch.float32).reshape(seq[0].weight.shape[0], -1)
            self._packed[name + "_lat"] = FoldedLinear(w[:, ks:], seq[0].bias, False, None, device)
            self._packed[name + "_small"] = w[:, :ks].contiguous().to(device)
            self._packed[name + "_rest"] = self._packed[name][1:]
        x = torch.linspace(-1, 1, dcd.grid_size)
        gx, gy = torch.meshgrid(x, x, indexing="ij")
        self._packed["grid"] = torch.stack([gx, gy], dim=-1).reshape(-1, 2).to(device)            # :82-88
        return self

    def _ensure_h2(self, device):
        """The f16x2 operands of the five planes stacks (three set-abstraction levels, the two FoldingNet chains), once per pack.  Every
        stack is bounded for a NORMALISED input -- features (post-ReLU maxima) in [0, 1], coordinates in [-1, 1] -- which forward()
        establishes per call from the data (pccx_absmax / pccx_dyn_scale: a power of two s <= 1 per stack, biases times s, outputs
        times 1 / s; Conv / ReLU stacks are positively homogeneous), so the interval bounds are rigorous whatever the input and restart
        at every stack: they stay within a few layers' looseness of the values (the lo pieces keep their bits)."""
        pk = self._packed
        if "h2" in pk:
            return pk["h2"]
        c_prev = 0
        for stack in pk["sa"]:
            h2_prepare_stack(stack, np.concatenate([np.zeros(c_prev), -np.ones(3)]), np.ones(c_prev + 3))   # :83 features first, xyz last
            c_prev = stack[-1].N
        for name in ("mlp1", "mlp2"):
            first, rest = pk[name][0], pk[name + "_rest"]
            h2_prepare_stack(rest, np.zeros(rest[0].K) if first.relu else -np.ones(rest[0].K), np.ones(rest[0].K))
        wsum = lambda w: float(np.abs(w.detach().cpu().numpy().astype(np.float64)).sum(axis=1).max() * 1.001)
        pk["h2"] = H2Scales(device, {"mlp1": wsum(pk["mlp1_small"]), "mlp2": wsum(pk["mlp2_small"])})
        return pk["h2"]

    def _splits(self, B):
        """FoldingNet's first layers can be evaluated as per-patch + per-point parts"""
        pk = self._packed
        return self.split_fold and B > 0 and _pow2x4(pk["mlp1"][0].N) and _pow2x4(pk["mlp2"][0].N)

    def _h2_eligible(self, B):
        """every planes stack of the forward has an f16x2 form: asked for, source-row levels, split folding"""
        pk = self._packed
        return (pk["sa"][0][0].planes_mode() == "f16x2" and PointnetSAModule.dedup and self._splits(B)
                and all(st[-1].N % 4 == 0 for st in pk["sa"]))

    def _fold(self, name, lat_dec, pts, mod, B, split, form, sc):
        """One folding MLP (PPPF_AE.py:99-107) on [pts | latent] -> (B * P, 3) rows.  pts: the grid (mod = P: the same for every patch) or
        the coarse points (mod = 0: one row each).  form: "f16x2" / "bf16x3" planes, or "rows" (fp32 rows layer by layer).
        split: the input [pts | latent] is never built: its 1024-wide latent part is the same for the P points of a patch, so the first
        layer is W_lat latent + bias once per PATCH (a Linear on B rows) plus a 2- / 3-term per-point update with ReLU, which on planes
        writes the next layer's operand PLANES directly (the fp32 rows of the 512-wide MLP were 1 GB written, read back and split per 2048
        patches); the remaining layers run on the P rows.  Otherwise the literal form, on planes without concatenating or repeating
        anything in memory (fold_planes), or on rows (:99-101, :106)."""
        pk, P = self._packed, self.decoder.num_points
        M = B * P
        with stage("fold_" + name):
            if not split:
                if form == "rows":
                    rep = lat_dec[:, None, :].expand(B, P, self.dim)
                    return pk[name].rows(cat_rows([pts[None].expand(B, P, -1) if mod else pts.view(B, P, -1), rep]))
                return run_planes(pk[name], fold_planes(pts, mod, lat_dec, P, M), M)
            base, rest, relu = pk[name + "_lat"](lat_dec), pk[name + "_rest"], pk[name][0].relu
            if form == "rows":
                return rest.rows(rows_affine_small(base, P, pts, mod, pk[name + "_small"], relu, M))
            rho = dyn = amax = None
            if form == "f16x2":
                # the chain's input relu(base + point part) is bounded from the data: max |base| + the per-point update's largest row sum
                # times max |point input| (the grid lies in [-1, 1], the coarse points' maximum comes out of the first chain's row epilogue)
                s_base, s_pts, s_dyn, s_out = self._FOLD_SLOTS[name]
                sc.absmax(base, s_base)
                if s_pts is None:
                    sc.scale(s_dyn, s_base, add=sc.wsum[name], comb=0)
                else:
                    sc.scale(s_dyn, s_base, s_pts, a2=sc.wsum[name], comb=0)
                rho, dyn, amax = rest[0].h2["sig"], sc.dy(s_dyn), sc.am(s_out)
            pl = rows_affine_small(base, P, pts, mod, pk[name + "_small"], relu, M, planes=form, rho=rho, dyn=dyn)
            return run_planes(rest, pl, M, ar=form, dyn=dyn, amax=amax)

    def forward(self, xyz):
        """xyz (B,N,3) on the GPU -> (recon (B,d*d,3), latent (B,dim), latent_quantized (B,d))."""
        if self._packed is None:
            self.pack(xyz.device)
        pk = self._packed
        B = xyz.shape[0]
        pts, feats = ops._f32c(xyz, "PPPF_AE"), None
        sc = None
        if self._h2_eligible(B):
            sc = self._ensure_h2(pts.device)
            sc.reset()
            sc.absmax(pts, 0)                                                       # max |coordinate|: every level's centroids are a subset
        for lvl, (mod, stack) in enumerate(zip((self.encoder.sa1, self.encoder.sa2, self.encoder.sa3), pk["sa"])):
            if sc is None:
                pts, feats = mod.run(stack, pts, feats)
                continue
            # the level's input = [maxima of the previous level's output rows, coordinates]: s from the larger of the two bounds
            sc.scale(lvl, lvl, 0 if lvl else None, a2=1.0 if lvl else 0.0)
            union = lvl == 2 and mod.union_max and pts.shape[1] in (32, 64, 128) and stack[-1].relu and not chain4_fits(stack)
            pts, feats = mod.run(stack, pts, feats, dyn=sc.dy(lvl), amax=sc.am(lvl + 1) if lvl < 2 else None,
                                 pad_out=lvl < 2 and PointnetSAModule.padded_levels, union=union)
        with stage("latent"):
            g = group_max(feats) if feats.dim() == 3 else feats                     # :44 max over the 32 points
            latent = sigmoid_spread(g, self.L)                                      # :136-137
            q = round_(pk["enc"](latent))                                           # :139-142
            lat_dec = pk["dec"](q)                                                  # :145
        # the FoldingNet form, chosen once: split or literal; f16x2 planes, bf16x3 planes, or fp32 rows (f32, and the empty batch)
        split = self._splits(B)
        form = "f16x2" if sc is not None else "bf16x3" if B > 0 and pk["mlp1"][0].mode() == "bf16x3" else "rows"
        x = self._fold("mlp1", lat_dec, pk["grid"], self.decoder.num_points, B, split, form, sc)   # :104 coarse
        x = self._fold("mlp2", lat_dec, x, 0, B, split, form, sc)                                   # :107 fine
        return x.view(B, self.decoder.num_points, 3), latent, q


def pppf_flops_per_patch(model, executed=False, n_points=512):
    """FLOPs (2 * MACs of every Conv / Linear, rows x in x out) of one PPPF_AE forward on one patch of n_points points.
    executed=False: as the reference evaluates it, every set-abstraction stack on its npoint x nsample grouped rows
    (pointnet_sa_module.py:86-90).  executed=True: what this implementation runs -- the stacks on the source rows only
    (PointnetSAModule.dedup), everything else unchanged."""
    if model._packed is None:
        raise _lib.PccxError("pppf_flops_per_patch: pack() the model first")
    pk, e = model._packed, model.encoder
    macs, n_src = 0, n_points
    for mod, stack in zip((e.sa1, e.sa2, e.sa3), pk["sa"]):
        rows = n_src if (executed and mod.dedup) else mod.npoint * mod.nsample
        macs += sum(rows * l.N * l.K for l in stack)
        n_src = mod.npoint
    macs += pk["enc"].N * pk["enc"].K + pk["dec"].N * pk["dec"].K
    P = model.decoder.num_points
    for name, ks in (("mlp1", 2), ("mlp2", 3)):
        st = pk[name]
        if executed and model.split_fold:
            macs += st[0].N * (st[0].K - ks) + P * st[0].N * ks + sum(P * l.N * l.K for l in st[1:])
        else:
            macs += sum(P * l.N * l.K for l in st)
    return 2 * macs


# =================================================================================================
# pppe PointCloudAE
# =================================================================================================
def _c2(in_c, out_c):
    return nn.Sequential(nn.Conv2d(in_c, out_c, 1, bias=False), nn.BatchNorm2d(out_c), nn.ReLU(inplace=True))


class PointNetSetAbstraction(nn.Module):                # pppe_pcd_ae.py:573-611
    def __init__(self, npoint, K, in_channel, mlp):
        super().__init__()
        self.npoint, self.K = npoint, K
        last = in_channel + 3
        layers = []
        for out in mlp:
            layers.append(_c2(last, out))
            last = out
        self.mlp_stack = nn.ModuleList(layers)

    def run(self, stack, xyz, feats, start, h2=None):
        """h2 = (H2Scales, amax slot of the offsets, amax slot of feats or None, dyn slot, amax slot of the output): the planes form in
        f16x2 -- `stack` is then the stack whose first layer is centred_first_layer() and h2_prepare_stack has run on it.  The grouped
        (B * S * K, 3 + C) rows never exist: the centred operand goes straight to planes, every layer runs on planes and the last one
        reduces over the K neighbours and folds the level's largest output for the next level."""
        B, N, _ = xyz.shape
        S = self.npoint
        new_xyz = xyz if S == N else ops.index_points(xyz, ops.farthest_point_sample_batch(xyz, S, start))   # :593-597
        nn_ = ops.knn_points(new_xyz, xyz, self.K, patch_scale=1.0)                  # :599-600 (nn - centre) * 1
        if h2 is not None:
            sc, a_off, a_feat, d, a_out = h2
            # s from the larger of the two input bounds; it has to exist before the first plane is written, so the offsets' maximum is
            # taken from the (B, S, K, 3) rows here and not from the operand kernel's own fold
            sc.absmax(nn_.knn, a_off)
            sc.scale(d, a_off, a_feat, a2=1.0 if a_feat is not None else 0.0)
            with stage("sa_stack_%d" % stack[-1].N):
                pl, rows = group_planes_centred(nn_.knn, feats, nn_.idx, "f16x2", stack[0].h2["sig"], sc.dy(d))   # :599-606
                y = run_planes(stack, pl, rows, "max", self.K, ar="f16x2", dyn=sc.dy(d), amax=sc.am(a_out))       # :607-610
            return new_xyz, y.view(B, S, -1)
        x = cat_rows([nn_.knn, ops.index_points(feats, nn_.idx)] if feats is not None else [nn_.knn])   # :606 xyz first
        return new_xyz, group_max(stack.rows(x).view(B * S, self.K, -1)).view(B, S, -1)   # :610


class PointNetSetAbstractionMSG(nn.Module):             # pppe_pcd_ae.py:614-632
    def __init__(self, npoint, scales, in_channel):
        super().__init__()
        self.branches = nn.ModuleList([PointNetSetAbstraction(npoint, s["K"], in_channel, s["mlp"]) for s in scales])


class PointNet2EncoderFull(nn.Module):                  # pppe_pcd_ae.py:637-667
    def __init__(self, latent_dim=256):
        super().__init__()
        self.sa_modules = nn.ModuleList([
            PointNetSetAbstractionMSG(512, [{"K": 16, "mlp": [32, 32, 64]}, {"K": 32, "mlp": [64, 64, 128]}], 0),
            PointNetSetAbstraction(128, 32, 64 + 128, [128, 128, 256]),
            PointNetSetAbstraction(32, 32, 256, [256, 256, 512])])
        self.global_conv = nn.Sequential(nn.Conv1d(512, 512, 1, bias=False), nn.BatchNorm1d(512), nn.ReLU(inplace=True),
                                         nn.Conv1d(512, latent_dim, 1))


class PCNDecoderSmall(nn.Module):                       # pppe_pcd_ae.py:691-707
    def __init__(self, latent_dim=256, coarse_points=512, final_points=8192):
        super().__init__()
        self.fc_coarse = nn.Sequential(nn.Linear(latent_dim, 512), nn.ReLU(), nn.Linear(512, coarse_points * 3))
        self.expansion_mlp = nn.Sequential(nn.Linear(coarse_points * 3 + latent_dim, 1024), nn.ReLU(),
                                           nn.Linear(1024, final_points * 3))
        self.coarse_points, self.final_points = coarse_points, final_points


class _PppeProbParams(nn.Module):                       # pppe_pcd_ae.py:751-772 (parameters only)
    def __init__(self, feature_dim=512, hidden_channels=128, latent_bins=16, latent_channels=3):
        super().__init__()
        self.cond_proj = nn.Sequential(nn.Linear(feature_dim, hidden_channels), nn.ReLU(), nn.Linear(hidden_channels, hidden_channels))
        self.combine = nn.Sequential(nn.Conv1d(latent_channels + hidden_channels, hidden_channels, 1), nn.ReLU(),
                                     nn.Conv1d(hidden_channels, hidden_channels, 1))
        self.mean_head = nn.Conv1d(hidden_channels, latent_channels, 1)
        self.scale_head = nn.Conv1d(hidden_channels, latent_channels, 1)
        self.pmf_head = nn.Conv1d(hidden_channels, latent_bins, 1)


class PointCloudAE(_Packable):
    """pppe_pcd_ae.PointCloudAE.forward (pppe_pcd_ae.py:843-877), eval mode."""

    # f16x2: every Conv / Linear stack of the forward on operand planes through run_planes (_forward_h2).  False = the rows path, which
    # is also what the f32 and bf16x3 modes run (f16x2 then means bf16x3 rows: FoldedLinear.mode).  True = the planes path for every
    # batch.  "auto" (the default) = whichever was measured faster for the batch: the planes path from h2_min_points input
    # points (B * N) on -- below that the forward is bound by its launches and the rows path is a few percent ahead.
    h2_stacks = "auto"
    h2_min_points = 16 * 8192
    # with h2_stacks: the three dense stacks after the encoder (gconv, coarse, expand; M = B rows) in f16x2 too; False leaves them on rows
    h2_tails = True
    # amax / dyn slots of the f16x2 forward (H2Scales).  Per set-abstraction stack: amax slot of its kNN offsets, amax slot of its input
    # features, its dyn slot, amax slot of its output.  The two MSG branches normalise separately and fold their outputs into ONE slot,
    # which so holds the larger of the two: the bound of the concatenated features level 1 reads.
    _SLOTS = {"msg0": (0, None, 0, 2), "msg1": (1, None, 1, 2), "sa1": (3, 2, 2, 4), "sa2": (5, 4, 3, 6)}
    _A_COARSE, _D_GCONV, _D_EXPAND, _N_AMAX, _N_DYN = 7, 4, 5, 8, 6

    def __init__(self, latent_dim=64, latent_bins=16, npoints=8192):
        super().__init__()
        self.encoder = PointNet2EncoderFull(latent_dim=latent_dim)
        self.decoder = PCNDecoderSmall(latent_dim=latent_dim, coarse_points=512, final_points=npoints)
        self.prob = _PppeProbParams(512, 128, latent_bins, latent_dim)
        self.latent_bins, self.latent_dim = latent_bins, latent_dim
        self.q_min, self.q_max = 0.0, latent_bins - 1.0
        self._packed = None

    def pack(self, device="cuda"):
        sa = self.encoder.sa_modules
        conv_bn_relu = lambda mods: Stack(FoldedLinear(l[0].weight, None, True, l[1], device) for l in mods)
        self._packed = dict(
            msg=[conv_bn_relu(br.mlp_stack) for br in sa[0].branches], sa1=conv_bn_relu(sa[1].mlp_stack), sa2=conv_bn_relu(sa[2].mlp_stack),
            gconv=_fold_stack(self.encoder.global_conv, device),
            coarse=_fold_stack(self.decoder.fc_coarse, device), expand=_fold_stack(self.decoder.expansion_mlp, device))
        return self

    def _ensure_h2(self, device):
        """The f16x2 operands of the planes stacks, once per pack.  Every stack is bounded for a NORMALISED input, which _forward_h2
        establishes per call from the data (a power of two s <= 1 per stack: biases times s, outputs times 1 / s):
          * the four set-abstraction stacks, their first layers repacked for the features-first planes of group_planes_centred:
            features (post-ReLU maxima) in [0, 1], offsets in [-1, 1];
          * gconv on the global maximum, in [0, 1];  coarse on y_deq, in [0, q_max] as it stands (no s);  expand on [coarse | y_deq],
            in [-1, 1] and [0, 1] after s from max|coarse| + q_max."""
        pk = self._packed
        if "h2" in pk:
            return pk["h2"]
        sa = self.encoder.sa_modules
        mods = dict(msg0=sa[0].branches[0], msg1=sa[0].branches[1], sa1=sa[1], sa2=sa[2])
        rows = dict(msg0=pk["msg"][0], msg1=pk["msg"][1], sa1=pk["sa1"], sa2=pk["sa2"])
        for name, mod in mods.items():
            first = mod.mlp_stack[0]
            st = Stack([centred_first_layer(first[0], first[1], device)] + rows[name].layers[1:])
            C = st[0].K - 3
            h2_prepare_stack(st, np.concatenate([np.zeros(C), -np.ones(3)]), np.ones(C + 3))
            pk[name + "_h2"] = st
        d, n_c = self.latent_dim, pk["coarse"][-1].N
        h2_prepare_stack(pk["gconv"], np.zeros(pk["gconv"][0].K), np.ones(pk["gconv"][0].K))
        h2_prepare_stack(pk["coarse"], np.zeros(d), np.full(d, self.q_max))
        h2_prepare_stack(pk["expand"], np.concatenate([-np.ones(n_c), np.zeros(d)]), np.ones(n_c + d))
        pk["h2"] = H2Scales(device, None, self._N_AMAX, self._N_DYN)
        return pk["h2"]

    def _forward_h2(self, x, starts):
        """forward() in the f16x2 arithmetic: the same selection kernels, every stack through run_planes."""
        pk, sa, B = self._packed, self.encoder.sa_modules, x.shape[0]
        sc = self._ensure_h2(x.device)
        sc.reset()
        outs, new_xyz = [], None
        for i, (br, st) in enumerate(zip(sa[0].branches, starts[0])):               # :617-632 (last branch's centroids win)
            new_xyz, f = br.run(pk["msg%d_h2" % i], x, None, st, h2=(sc,) + self._SLOTS["msg%d" % i])
            outs.append(f)
        feats = torch.cat(outs, dim=-1).contiguous()
        xyz, feats = sa[1].run(pk["sa1_h2"], new_xyz, feats, starts[1], h2=(sc,) + self._SLOTS["sa1"])
        xyz, feats = sa[2].run(pk["sa2_h2"], xyz, feats, starts[2], h2=(sc,) + self._SLOTS["sa2"])
        cond = group_max(feats)                                                      # :682 global max
        tails = self.h2_tails

        def dense(name, f0, f1=None, dyn=None, amax=None):
            """one dense stack on B rows: [f0 | f1] -> planes -> run_planes (rows)"""
            if not tails:
                return pk[name].rows(f0 if f1 is None else torch.cat([f0, f1], dim=1).contiguous())
            pl, _ = group_planes(f0, f1, ar="f16x2", sig=pk[name][0].h2["sig"], dyn=dyn)
            return run_planes(pk[name], pl, B, ar="f16x2", dyn=dyn, amax=amax)

        if tails:
            sc.scale(self._D_GCONV, self._SLOTS["sa2"][3])                          # max cond = the largest output of the last level
        latent = dense("gconv", cond, dyn=sc.dy(self._D_GCONV))                      # :684
        y_q, y_deq = torch.empty_like(latent), torch.empty_like(latent)
        _lib.call("pccx_quantize_st", latent.data_ptr(), latent.numel(), float(self.q_min), float(self.q_max),
                  int(self.latent_bins), y_q.data_ptr(), y_deq.data_ptr(), _stream())
        c = dense("coarse", y_deq, amax=sc.am(self._A_COARSE))                       # :710; y_deq lies in [0, q_max]: no s
        if tails:
            sc.scale(self._D_EXPAND, self._A_COARSE, add=self.q_max, comb=0)         # |[coarse | y_deq]| <= max|coarse| + q_max
        e = dense("expand", c, y_deq, dyn=sc.dy(self._D_EXPAND))                     # :711-712
        return c.view(B, -1, 3), e.view(B, -1, 3), cond, y_q, latent

    def forward(self, x, starts):
        """x (B,N,3) on the GPU; starts = [[msg_branch0, msg_branch1], sa2, sa3], each (B,) FPS start
        indices (the reference draws them with torch.randint, pn_kit.py:321).
        -> (coarse (B,512,3), fine (B,N,3), cond_feats (B,512), y_q (B,d), latent (B,d))."""
        if self._packed is None:
            self.pack(x.device)
        pk = self._packed
        x = ops._f32c(x, "PointCloudAE")
        B = x.shape[0]
        h2 = B * x.shape[1] >= self.h2_min_points if self.h2_stacks == "auto" else bool(self.h2_stacks)
        if h2 and B > 0 and _arith() == "f16x2":
            return self._forward_h2(x, starts)
        sa = self.encoder.sa_modules
        outs, new_xyz = [], None
        for br, stack, st in zip(sa[0].branches, pk["msg"], starts[0]):             # :617-632 (last branch's centroids win)
            new_xyz, f = br.run(stack, x, None, st)
            outs.append(f)
        feats = torch.cat(outs, dim=-1).contiguous()
        xyz, feats = sa[1].run(pk["sa1"], new_xyz, feats, starts[1])
        xyz, feats = sa[2].run(pk["sa2"], xyz, feats, starts[2])
        cond = group_max(feats)                                                      # :682 global max
        latent = pk["gconv"].rows(cond)                                              # :684
        # quantize_st (:719-735) then dequantise (:873); the mean over N tiled copies (:875) is the value itself
        y_q, y_deq = torch.empty_like(latent), torch.empty_like(latent)
        _lib.call("pccx_quantize_st", latent.data_ptr(), latent.numel(), float(self.q_min), float(self.q_max),
                  int(self.latent_bins), y_q.data_ptr(), y_deq.data_ptr(), _stream())
        c = pk["coarse"].rows(y_deq)                                                 # :710
        e = pk["expand"].rows(torch.cat([c, y_deq], dim=1).contiguous())             # :711-712
        return c.view(B, -1, 3), e.view(B, -1, 3), cond, y_q, latent
