"""Host-side mirror of the reference's model classes (AE.py, pn_kit.py) over libpccx.so.

The classes keep the reference's constructor arguments and ``state_dict`` key names (SURVEY
Appendix C) so reference checkpoints load with ``load_state_dict``; torch modules are used as
parameter containers only.  Every forward computation is a HIP kernel behind the C ABI; there
is no torch / CPU compute path (inference only, as compress.py / decompress.py use the models).
"""
import torch
import torch.nn as nn

from . import _lib, MATMUL_MODES
from .ops import _stream, _f32c, stage


def check_matmul(name, value):
    if value not in MATMUL_MODES:
        raise ValueError(f"{name}={value!r}: expected 'f32', 'bf16x3' or 'f16x2'")


def _conv_stack(chans, relu):
    mods = nn.ModuleList()
    for i in range(len(chans) - 1):
        layers = [nn.Conv2d(chans[i], chans[i + 1], 1)]
        if relu[i]:
            layers.append(nn.ReLU())
        mods.append(nn.Sequential(*layers))
    return mods


def _pccx_default_matmul():
    from . import DEFAULT_MATMUL
    return DEFAULT_MATMUL


def _folded(conv, relu, device):
    from .families import FoldedLinear          # generic runtime-shaped fp32 MFMA layer (csrc/linear.hip)
    return FoldedLinear(conv.weight, conv.bias, relu, None, device)


def _folded_sequence(mods, device):
    """The Linear / 1x1 Conv2d modules of a Sequential's list as generic layers, each with the ReLU that follows it fused."""
    return [_folded(m, i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU), device)
            for i, m in enumerate(mods) if isinstance(m, (nn.Linear, nn.Conv2d))]


def _lazy_layers(module, device, build):
    """module._layers = (device, build(device)): the generic path's packed layers, built on first use on a device.  The owner's
    load_state_dict drops them by setting _layers to None."""
    device = torch.device(device)
    if module._layers is None or module._layers[0] != device:
        object.__setattr__(module, "_layers", (device, build(device)))      # not a sub-module / buffer: plain attribute
    return module._layers[1]


class _Params(nn.Module):
    """Sub-modules of the reference's models.  They hold the parameters under the reference's state_dict keys AND are
    callable like the reference's (compress.py:113-121 calls ae.sa(x) / ae.pn(x), decompress.py:97-101 ae.inv_pool /
    ae.inv_mlp): forward runs HIP kernels -- the owning AE's fused entry points when the module is one of AE's and the
    shapes are the fused kernel's, otherwise the generic layer kernels (pccx_linear / pccx_group_max).  No torch compute."""

    _fused = None                 # set by the owning AE: a callable taking the reference's arguments, or None
    _layers = None                # generic path: packed layers, built lazily on the input's device

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._layers = None
        return r

    def _own(self, fused):
        object.__setattr__(self, "_fused", fused)      # not a sub-module / buffer: plain attribute


class _ConvStack(_Params):
    def _stack(self, device):
        return _lazy_layers(self, device, lambda dev: [_folded(m[0], len(m) > 1, dev) for m in self.mlp_Modules])

    def _rows(self, points):
        x = _f32c(points, type(self).__name__)
        if x.dim() != 3:
            raise _lib.PccxError(f"{type(self).__name__}: expected [B, C, N], got {tuple(x.shape)}")
        B, Cc, N = x.shape
        rows = x.permute(0, 2, 1).reshape(B * N, Cc).contiguous()          # channels-last rows
        for layer in self._stack(x.device):
            rows = layer(rows)
        return rows, B, N


class SetAbstraction(_Params):      # pn_kit.SetAbstraction (pn_kit.py:146-161), bn=False
    def __init__(self, npoint, K, in_channel, mlp, bn=False, finalRelu=True):
        super().__init__()
        if bn:
            raise _lib.PccxError("pccx.SetAbstraction: bn=True is not on the codec path (AE.py:16 uses bn=False)")
        self.npoint, self.K, self.finalRelu = npoint, K, finalRelu
        self.conv0 = nn.Conv2d(in_channel + 3, mlp[0], 1)
        self.conv1 = nn.Conv2d(mlp[0], mlp[1], 1)
        self.conv2 = nn.Conv2d(mlp[1], mlp[2], 1)

    def forward(self, xyz, start_idx=None):
        """pn_kit.SetAbstraction.forward (pn_kit.py:164-211): xyz [B, 3, N] -> (new_xyz [B, 3, S], new_points [B, D', S])."""
        x = _f32c(xyz, "SetAbstraction")
        B, Cc, N = x.shape
        if self._fused is not None and self.npoint == N and Cc == 3:
            return self._fused(x)
        from .families import group_max
        from . import ops
        pts = x.permute(0, 2, 1).contiguous()                                              # :173
        S = self.npoint
        new_xyz = pts if S == N else ops.index_points(pts, ops.farthest_point_sample_batch(pts, S, start_idx))   # :180-183
        nn_ = ops.knn_points(new_xyz, pts, self.K, patch_scale=1.0)                        # :190-191 (nn - centre)
        rows = nn_.knn.reshape(B * S * self.K, Cc).contiguous()
        for layer in _lazy_layers(self, x.device, lambda dev: [_folded(self.conv0, True, dev), _folded(self.conv1, True, dev),
                                                               _folded(self.conv2, self.finalRelu, dev)]):
            rows = layer(rows)                                                             # :198-205
        feat = group_max(rows.view(B * S, self.K, -1)).view(B, S, -1)                      # :207
        return new_xyz.permute(0, 2, 1), feat.permute(0, 2, 1)                             # :209-211


class PointNet(_ConvStack):         # pn_kit.PointNet (pn_kit.py:98-121), bn=False
    def __init__(self, in_channel, mlps, relu, bn=False):
        super().__init__()
        if bn:
            raise _lib.PccxError("pccx.PointNet: bn=True is not on the codec path (AE.py:17 uses bn=False)")
        self.mlp_Modules = _conv_stack([in_channel] + list(mlps), relu)

    def forward(self, points):
        """pn_kit.PointNet.forward (pn_kit.py:124-144): points [B, C, N] -> [B, D] (max over the N points)."""
        if self._fused is not None:
            r = self._fused(points)
            if r is not None:
                return r
        from .families import group_max
        rows, B, N = self._rows(points)
        return group_max(rows.view(B, N, -1))


class MLP(_ConvStack):              # pn_kit.MLP (pn_kit.py:263-286), bn=False
    def __init__(self, in_channel, mlps, relu, bn=False):
        super().__init__()
        if bn:
            raise _lib.PccxError("pccx.MLP: bn=True is not on the codec path (AE.py:27 uses bn=False)")
        self.mlp_Modules = _conv_stack([in_channel] + list(mlps), relu)

    def forward(self, points):
        """pn_kit.MLP.forward (pn_kit.py:288-305): points [B, C, N] -> [B, D, N]."""
        rows, B, N = self._rows(points)
        return rows.view(B, N, -1).permute(0, 2, 1)


class LinearStack(nn.Sequential):
    """nn.Sequential of Linear / ReLU (AE.py:19-26 inv_pool) with the reference's state_dict keys; forward = one
    pccx_linear launch per Linear (ReLU fused)."""

    _layers = None

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._layers = None
        return r

    def forward(self, x):
        x = _f32c(x, "inv_pool")
        lead = x.shape[:-1]
        rows = x.reshape(-1, x.shape[-1]).contiguous()
        for layer in _lazy_layers(self, x.device, lambda dev: _folded_sequence(list(self), dev)):
            rows = layer(rows)
        return rows.view(*lead, -1)


def _host(t):
    return t.detach().to("cpu", torch.float32).contiguous()


_WS = {}


def workspace(tag, numel, device):
    """Persistent scratch buffers (HBM is 288 GB: keep the big intermediates resident instead of going
    through the allocator every call).  Stream-ordered reuse is safe: every consumer of a buffer is
    enqueued before its next producer on the same stream."""
    key = (tag, str(device), torch.cuda.current_stream().cuda_stream)      # one buffer per stream: streams run concurrently
    t = _WS.get(key)
    if t is None or t.numel() < numel:
        _WS[key] = t = torch.empty(int(numel), device=device, dtype=torch.float32)
    return t[:numel]


def _pack(fn_name, size, tensors, ints):
    keep = [_host(t) for t in tensors]
    blob = torch.zeros(size, dtype=torch.float32)
    _lib.call(fn_name, *[t.data_ptr() for t in keep], *ints, blob.data_ptr())
    return blob


def _pack_on_device(fn_name, size, src, ints=()):
    """A blob of bf16x3 planes built by a kernel from the packed fp32 blob ``src`` (csrc/pack.hip)."""
    blob = torch.empty(size, device=src.device, dtype=torch.float32)
    _lib.call(fn_name, src.data_ptr(), *ints, blob.data_ptr(), _stream())
    return blob


# The blobs derived from the packed pair (enc, dec) of an AE: name -> builder(ae, lib, enc, dec).  The bf16x3 planes come from the fp32
# blobs on the device, the f16x2 ones are packed on the host from the weights (csrc/pack_h2.hip) and uploaded.
_DERIVED_BLOBS = {
    "sa_b3": lambda ae, lib, enc, dec: _pack_on_device("pccx_pack_sa_b3", lib.pccx_sa_b3_blob_floats(), enc),
    "pn_b3": lambda ae, lib, enc, dec: _pack_on_device("pccx_pack_pn_b3", lib.pccx_pn_b3_blob_floats(), enc),
    "dec_b3": lambda ae, lib, enc, dec: _pack_on_device("pccx_pack_ae_decoder_b3", lib.pccx_dec_b3_blob_floats(ae.k), dec, (ae.k,)),
    "enc_h2": lambda ae, lib, enc, dec: _pack("pccx_pack_ae_encoder_h2", lib.pccx_ae_encoder_h2_blob_floats(), ae._enc_tensors(),
                                              [ae.d]).to(enc.device),
    "dec_h2": lambda ae, lib, enc, dec: _pack("pccx_pack_ae_decoder_h2", lib.pccx_ae_decoder_h2_blob_floats(ae.k), ae._dec_tensors(),
                                              [ae.k, ae.d]).to(enc.device),
}
# The fused encoders: mode -> (entry point taking the in-patch neighbour tables, its workspace size function, derived blobs after enc_blob,
# whether it takes the list of distinct patches)
_FUSED_ENCODERS = {
    "f16x2": ("pccx_ae_encode_h2_tables_list", "pccx_ae_encode_h2_workspace_bytes", ("enc_h2",), True),
    "bf16x3": ("pccx_ae_encode_b3_tables", "pccx_ae_encode_b3_workspace_bytes", ("sa_b3", "pn_b3"), False),
}
# The decoders: mode -> (entry point, workspace size function, tag of the persistent workspace, derived blob after dec_blob)
_DECODERS = {
    "f32": ("pccx_ae_decode", "pccx_ae_decode_workspace_floats", "dec_h2", None),
    "bf16x3": ("pccx_ae_decode_b3", "pccx_ae_decode_b3_workspace_floats", "dec_h2_b3", "dec_b3"),
    "f16x2": ("pccx_ae_decode_h2_list", "pccx_ae_decode_h2_workspace_floats", "dec_h2_h2", "dec_h2"),
}


class AE(nn.Module):
    """AE.AE (AE.py:12-55): SetAbstraction + PointNet encoder, Linear + MLP decoder."""

    def __init__(self, K, k, d, L):
        super().__init__()
        if d < 1 or L < 1 or K % 16 != 0 or not 16 <= K <= 1024:
            raise _lib.PccxError(
                f"pccx.AE: --K must be a multiple of 16 in 16..1024 (got {K}; the reference's octree rate table pn_kit.py:17-23 has "
                f"64..1024 only) and --d, --L positive (got {d}, {L}); the reference's defaults are --K 256 --d 16 --L 7 "
                f"(compress.py:30-34)")
        # the fused transforms cover the bottleneck widths --d 1..16; wider ones (compress.py:31 accepts any) run PointNet and the
        # decoder through the generic layer kernels, chunked over the patches (correct and slow: encode_generic / decode_generic)
        self.fused_d = d <= 16
        self.sa = SetAbstraction(npoint=K, K=16, in_channel=0, mlp=[32, 64, 128])
        self.pn = PointNet(3 + 128, [128, 256, 512, d], [True, True, True, False])
        self.inv_pool = LinearStack(nn.Linear(d, 256), nn.ReLU(), nn.Linear(256, 1024), nn.ReLU(),
                                    nn.Linear(1024, k * 128), nn.ReLU())
        self.inv_mlp = MLP(d + 128, [128, 64, 32, 3], [True, True, True, False])
        self.K, self.k, self.d, self.L = K, k, d, L
        self._enc_blob = self._dec_blob = None
        self._derived_blobs = {}
        self.sa._own(self._sa_call)
        self.pn._own(self._pn_call)

    def quantize(self, x):          # AE.STEQuantize.forward (AE.py:79-81); straight-through gradient (AE.py:83-85)
        from .ops import ste_round
        return ste_round(x)

    # ---- the reference's per-module calls (compress.py:113-121), on the fused kernels ----------------------------
    def _sa_call(self, x):
        """ae.sa(x): x [P, 3, K] -> (new_xyz [P, 3, K] (= x, npoint == K, pn_kit.py:180-181), features [P, 128, K])."""
        P, _, K = x.shape
        if K % 16 != 0 or not 16 <= K <= 1024:
            raise _lib.PccxError(f"ae.sa: K={K} must be a multiple of 16 in 16..1024")
        patches = x.permute(0, 2, 1).contiguous()
        feat = torch.empty(P, 8, K, 16, device=x.device, dtype=torch.float32)
        self._launch_sa(patches, feat, _pccx_default_matmul())
        return x, feat.permute(0, 1, 3, 2).reshape(P, 128, K)

    def _pn_call(self, points):
        """ae.pn(cat(x_patches, features)): [P, 3 + 128, K] -> raw latent [P, d] (before the sigmoid of compress.py:126)."""
        x = _f32c(points, "ae.pn")
        if not self.fused_d or x.dim() != 3 or x.shape[1] != 131 or x.shape[2] % 16 != 0 or not 16 <= x.shape[2] <= 1024:
            return None                                   # not the fused kernel's shape: generic path
        P, _, K = x.shape
        patches = x[:, :3].permute(0, 2, 1).contiguous()
        feat = x[:, 3:].reshape(P, 8, 16, K).permute(0, 1, 3, 2).contiguous()
        outs = [torch.empty(P, self.d, device=x.device, dtype=torch.float32) for _ in range(3)]
        self._launch_pn(patches, feat, outs, _pccx_default_matmul())
        return outs[0]

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._enc_blob = self._dec_blob = None
        self._derived_blobs.clear()
        return r

    def pack(self, device="cuda"):
        """Build the MFMA fragment blobs (C ABI pccx_pack_*) and upload them."""
        lib = _lib.load()
        tensors, d = self._enc_tensors(), self.d
        if not self.fused_d:
            # only the SetAbstraction part of the encoder blob is used (ae.sa does not depend on --d): pack it with a 16-wide stand-in
            # for PointNet's last layer; PointNet and the decoder run through the generic layers (their own lazily packed weights)
            tensors, d = tensors[:12] + [torch.zeros(16, 512), torch.zeros(16)], 16
        self._enc_blob = _pack("pccx_pack_ae_encoder", lib.pccx_ae_encoder_blob_floats(), tensors, [d]).to(device)
        self._dec_blob = _pack("pccx_pack_ae_decoder", lib.pccx_ae_decoder_blob_floats(self.k), self._dec_tensors(),
                               [self.k, self.d]).to(device) if self.fused_d else None
        self._derived_blobs.clear()
        for m in (self.sa, self.pn, self.inv_pool, self.inv_mlp):         # the generic path's packed copies: rebuilt on their next use
            m._layers = None
        return self

    def _enc_tensors(self):
        sd = self.state_dict()
        w = lambda key: sd[key].reshape(sd[key].shape[0], -1)
        return [w("sa.conv0.weight"), sd["sa.conv0.bias"], w("sa.conv1.weight"), sd["sa.conv1.bias"],
                w("sa.conv2.weight"), sd["sa.conv2.bias"],
                w("pn.mlp_Modules.0.0.weight"), sd["pn.mlp_Modules.0.0.bias"],
                w("pn.mlp_Modules.1.0.weight"), sd["pn.mlp_Modules.1.0.bias"],
                w("pn.mlp_Modules.2.0.weight"), sd["pn.mlp_Modules.2.0.bias"],
                w("pn.mlp_Modules.3.0.weight"), sd["pn.mlp_Modules.3.0.bias"]]

    def _dec_tensors(self):
        sd = self.state_dict()
        w = lambda key: sd[key].reshape(sd[key].shape[0], -1)
        return [sd["inv_pool.0.weight"], sd["inv_pool.0.bias"], sd["inv_pool.2.weight"], sd["inv_pool.2.bias"],
                sd["inv_pool.4.weight"], sd["inv_pool.4.bias"],
                w("inv_mlp.mlp_Modules.0.0.weight"), sd["inv_mlp.mlp_Modules.0.0.bias"],
                w("inv_mlp.mlp_Modules.1.0.weight"), sd["inv_mlp.mlp_Modules.1.0.bias"],
                w("inv_mlp.mlp_Modules.2.0.weight"), sd["inv_mlp.mlp_Modules.2.0.bias"],
                w("inv_mlp.mlp_Modules.3.0.weight"), sd["inv_mlp.mlp_Modules.3.0.bias"]]

    def _blobs(self, device):
        if self._enc_blob is None or self._enc_blob.device != torch.device(device):
            self.pack(device)
        return self._enc_blob, self._dec_blob

    def _derived(self, name, device):
        """One of the five blobs made from the packed weights, built on first use on a device; pack() and load_state_dict() drop them."""
        enc, dec = self._blobs(device)                    # first: packing for another device empties the cache
        blob = self._derived_blobs.get(name)
        if blob is None or blob.device != enc.device:
            blob = self._derived_blobs[name] = _DERIVED_BLOBS[name](self, _lib.load(), enc, dec)
        return blob

    def _sa_b3_blob(self, device):
        """bf16x3 planes of the SetAbstraction conv1 / conv2 weights."""
        return self._derived("sa_b3", device)

    def _pn_b3_blob(self, device):
        """bf16x3 planes of the PointNet weight stream."""
        return self._derived("pn_b3", device)

    def _dec_b3_blob(self, device):
        """bf16x3 planes of the decoder's big Linear."""
        return self._derived("dec_b3", device)

    def _enc_h2_blob(self, device):
        """f16x2 operand planes, scaled biases and layer scales of the encoder."""
        return self._derived("enc_h2", device)

    def _dec_h2_blob(self, device):
        return self._derived("dec_h2", device)

    def _launch_sa(self, x, feat, matmul):
        P, K, _ = x.shape
        enc, _ = self._blobs(x.device)
        check_matmul("sa_matmul", matmul)
        if matmul == "f32":
            _lib.call("pccx_sa_forward", x.data_ptr(), P, K, enc.data_ptr(), feat.data_ptr(), _stream())
        else:                                             # f16x2 exists for the fused transforms only: the module alone runs bf16x3
            _lib.call("pccx_sa_forward_b3", x.data_ptr(), P, K, enc.data_ptr(), self._sa_b3_blob(x.device).data_ptr(),
                      feat.data_ptr(), _stream())

    def _launch_pn(self, x, feat, outs, matmul):
        P, K, _ = x.shape
        enc, _ = self._blobs(x.device)
        check_matmul("pn_matmul", matmul)
        if matmul == "f32":
            _lib.call("pccx_pn_forward", x.data_ptr(), feat.data_ptr(), P, K, enc.data_ptr(), self.d, self.L,
                      outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), _stream())
        else:
            _lib.call("pccx_pn_forward_b3", x.data_ptr(), feat.data_ptr(), P, K, enc.data_ptr(), self._pn_b3_blob(x.device).data_ptr(),
                      self.d, self.L, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), _stream())

    def encode(self, patches, sa_matmul=None, pn_matmul=None, fused=True, groups=None):
        """patches (BS,K,3), centred and scaled -> (latent_raw, latent, latent_quantized), each (BS,d).
        = ae.sa + ae.pn + sigmoid spread + round (compress.py:113-127, AE.py:37-45).
        sa_matmul / pn_matmul: "f32" (exact-fp32 MFMA), "bf16x3" (fp32 products of three bf16 pieces per operand on the
        bf16 matrix cores) or "f16x2" (two exactly scaled fp16 pieces per operand, three products on the fp16 matrix cores;
        both split modes: fp32-level error, a latent within ~1e-6 of a rounding boundary may round the other way);
        None = pccx.DEFAULT_MATMUL.  "f16x2" exists as the fused kernel only (it holds every K up to 1024): with fused=False or different modes
        for the two modules, an "f16x2" request runs the bf16x3 kernels.  fused=False forces the
        two-kernel path (feature map through HBM).
        groups (ops.patch_groups over the patches' centres): the patches with groups.rep[p] != p are copies of patch rep[p] (their rows of
        `patches` need not even be filled in).  The fused f16x2 kernels then transform the representatives only; every path ends by copying
        the representatives' three latent rows to their copies, so the results are complete (P, d) arrays either way."""
        x = _f32c(patches, "AE.encode")
        outs = self._encode(x, sa_matmul, pn_matmul, fused, groups)
        if groups is not None:
            from .ops import replicate_rows
            replicate_rows(groups, *outs)
        return outs

    def _encode(self, x, sa_matmul, pn_matmul, fused, groups):
        P, K, _ = x.shape
        if groups is not None and groups.rep.numel() != P:
            raise _lib.PccxError(f"AE.encode: groups of {groups.rep.numel()} patches for {P} patches")
        if not self.fused_d:
            return self.encode_generic(x)
        outs = [torch.empty(P, self.d, device=x.device, dtype=torch.float32) for _ in range(3)]
        sa_matmul, pn_matmul = sa_matmul or _pccx_default_matmul(), pn_matmul or _pccx_default_matmul()
        lib = _lib.load()
        # one kernel, the (P,128,K) feature map never leaves the CU: on f16x2 operands (csrc/encoder_fused_h2.hip) when both modules ask
        # for them; every other f16x2 request runs bf16x3, fused (csrc/encoder_fused.hip) when both modules then agree on it
        if fused and sa_matmul == pn_matmul == "f16x2" and lib.pccx_ae_encode_h2_fused_ok(K):
            mode = "f16x2"
        else:
            sa_matmul, pn_matmul = ("bf16x3" if m == "f16x2" else m for m in (sa_matmul, pn_matmul))
            mode = "bf16x3" if fused and sa_matmul == pn_matmul == "bf16x3" and lib.pccx_ae_encode_b3_fused_ok(K) else None
        if mode is not None:
            tables_fn, ws_bytes, blobs, takes_lists = _FUSED_ENCODERS[mode]
            enc, _ = self._blobs(x.device)
            # the in-patch 16-NN tables come from a kernel of their own (csrc/patch_knn.hip) through a persistent workspace, 4 KB per
            # 256-point patch: two calls, so that a stage timer sees each kernel on its own
            ws = workspace("patch_knn16", (getattr(lib, ws_bytes)(P, K) + 3) // 4, x.device)
            lists = (groups.uniq.data_ptr(), groups.n_uniq.data_ptr()) if takes_lists and groups is not None else (None, None)
            with stage("patch_knn16"):
                _lib.call("pccx_patch_knn16_list", x.data_ptr(), P, K, ws.data_ptr(), *lists, _stream())
            with stage("sa_pn_forward"):
                _lib.call(tables_fn, x.data_ptr(), P, K, enc.data_ptr(), *[self._derived(b, x.device).data_ptr() for b in blobs],
                          self.d, self.L, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(),
                          *(lists if takes_lists else ()), _stream())
            return tuple(outs)
        # the two-kernel path, the feature map through HBM
        ws = workspace("sa_feat", P * K * 128, x.device)
        with stage("sa_forward"):
            self._launch_sa(x, ws, sa_matmul)
        with stage("pn_forward"):
            self._launch_pn(x, ws, outs, pn_matmul)
        return tuple(outs)

    def encode_generic(self, x, chunk=1024):
        """encode() for bottleneck widths the fused PointNet does not cover (--d > 16): ae.sa on its kernel (it does not depend on d),
        ae.pn through the generic layers (pccx_linear* + pccx_group_max), sigmoid spread and round by their kernels -- the statement
        sequence of compress.py:113-127, ``chunk`` patches at a time (the (chunk, K, 131) rows are the memory bound)."""
        from .families import sigmoid_spread, round_
        raws = []
        for i in range(0, x.shape[0], chunk):
            xt = x[i:i + chunk].permute(0, 2, 1).contiguous()                  # (p, 3, K)
            _, feat = self.sa(xt)                                              # compress.py:113-115
            raws.append(self.pn(torch.cat((xt, feat), dim=1)))                 # compress.py:116-121
        raw = torch.cat(raws) if raws else torch.empty(0, self.d, device=x.device)
        latent = sigmoid_spread(raw, self.L)                                   # AE.py:43-44
        return raw, latent, round_(latent)                                     # AE.py:45

    def decode_generic(self, q, chunk=1024):
        """latent_q (P, d) -> raw decoder output (P, k, 3) through ae.inv_pool / ae.inv_mlp on the generic layers
        (decompress.py:97-102), ``chunk`` patches at a time (inv_pool's (chunk, k * 128) rows are the memory bound)."""
        outs = []
        for i in range(0, q.shape[0], chunk):
            lq = q[i:i + chunk]
            lin = self.inv_pool(lq).view(lq.shape[0], -1, self.k)                                  # :97-98
            mlp_in = torch.cat((lin, lq.unsqueeze(-1).tile((1, 1, self.k))), dim=1)                # :99-100
            outs.append(self.inv_mlp(mlp_in).transpose(2, 1).contiguous())                         # :101-102
        return torch.cat(outs) if outs else torch.empty(0, self.k, 3, device=q.device)

    def decode(self, latent_q, centres=None, center=None, longest=None, S=None, scale=None, margin=0.01, matmul=None, group=False, short_list=False,
               groups=None):
        """latent_q (BS,d) -> decoded patches (BS,k,3) (AE.py:48-53).  With centres/center/longest/S/scale
        it returns instead the reassembled, denormalised cloud (B,S*k,3) of decompress.py:104-116.
        matmul="bf16x3" / "f16x2" evaluate the matrix products as fp32 products of three bf16 / two exactly scaled fp16 pieces
        per operand on the matrix cores (fp32-level error, not bit-identical to "f32"); None = pccx.DEFAULT_MATMUL.
        group=True (reassembling form, "f16x2"): patches of a cloud with the same (centre row, latent_q row) decode to the same 3 k floats, so
        the decoder runs once per distinct pair (ops.patch_groups) and the copies are filled from it; the other modes decode every patch.
        short_list=True (with group): the caller expects far fewer distinct pairs than patches (octree_mode "reference"), and the head runs in
        its one-tile-per-workgroup form; same result.
        groups (raw-patches form, "f16x2"; the ragged path): ops.patch_groups the caller made over its (centre row, latent_q row) keys --
        the listed patches are decoded and the copies filled from them; the other modes decode every patch."""
        matmul = matmul or _pccx_default_matmul()
        q = _f32c(latent_q, "AE.decode")
        P = q.shape[0]
        reassemble = centres is not None
        if not (self.fused_d or reassemble):
            return self.decode_generic(q)
        if reassemble:
            B = P // S
            centres = _f32c(centres.reshape(P, 3), "AE.decode.centres")
            center = _f32c(center.reshape(B, 3), "AE.decode.center")
            longest = _f32c(longest.reshape(B), "AE.decode.longest")
            form = (float(scale), centres.data_ptr(), center.data_ptr(), longest.data_ptr(), int(S), float(margin))
            result = torch.empty(B, S * self.k, 3, device=q.device, dtype=torch.float32)
        else:
            form = (0.0, None, None, None, 1, float(margin))
            result = torch.empty(P, self.k, 3, device=q.device, dtype=torch.float32)
        if not self.fused_d:
            raw = self.decode_generic(q)
            _lib.call("pccx_reassemble", raw.data_ptr(), P, self.k, *form, result.data_ptr(), _stream())
            return result
        check_matmul("matmul", matmul)
        fn, ws_floats, ws_tag, blob = _DECODERS[matmul]
        _, dec = self._blobs(q.device)
        extra = (self._derived(blob, q.device).data_ptr(),) if blob else ()
        ws = workspace(ws_tag, getattr(_lib.load(), ws_floats)(P), q.device)
        groups, lists = (None if reassemble else groups), ()
        if groups is not None and groups.rep.numel() != P:
            raise _lib.PccxError(f"AE.decode: groups of {groups.rep.numel()} patches for {P} patches")
        if matmul != "f16x2":
            groups = None
        else:
            if group and reassemble:
                from .ops import patch_groups, replicate_rows
                groups = patch_groups(centres.view(B, S, 3), q.view(B, S, self.d))
            lists = (groups.uniq.data_ptr(), groups.n_uniq.data_ptr()) if groups is not None else (None, None)
        # patches_out, then the reassembling arguments, then pc_out: one of the two destinations is null
        dest = (None, *form, result.data_ptr()) if reassemble else (result.data_ptr(), *form, None)
        if groups is not None and short_list:
            fn = "pccx_ae_decode_h2_short_list"
        _lib.call(fn, q.data_ptr(), P, self.d, self.k, dec.data_ptr(), *extra, ws.data_ptr(), *dest, *lists, _stream())
        if groups is not None:
            from .ops import replicate_rows
            replicate_rows(groups, result)
        return result

    def forward(self, xyz):
        """AE.AE.forward (AE.py:34-55), inference: xyz (BS,K,3) -> (new_xyz (BS,k,3), latent, latent_quantized)."""
        _, latent, q = self.encode(xyz)
        return self.decode(q), latent, q


class ConditionalProbabilityModel(nn.Module):
    """AE.ConditionalProbabilityModel (AE.py:87-123)."""

    _layers = None                # generic path: model_mlp's packed layers (_lazy_layers)

    def __init__(self, L, d):
        super().__init__()
        self.L, self.d = L, d
        self.model_pn = PointNet(3, [64, 128, 256], [True, True, True])
        self.model_mlp = nn.Sequential(nn.Conv2d(3 + 256, 512, 1), nn.ReLU(), nn.Conv2d(512, 512, 1), nn.ReLU(),
                                       nn.Conv2d(512, d * L, 1))
        self._blob = None

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._blob = self._layers = self.model_pn._layers = None      # model_pn's weights came in through this call too
        return r

    def fused_ok(self, S=16):
        """The fused kernel covers d <= 16, L <= 15, d * L <= 128 and S a multiple of 16; everything else takes the generic layers."""
        return self.d <= 16 and self.L <= 15 and self.d * self.L <= 128 and S % 16 == 0 and S >= 16

    def pack(self, device="cuda"):
        self._layers = self.model_pn._layers = None                   # the generic path's packed copies: rebuilt on their next use
        if not self.fused_ok():
            self._blob = None
            return self
        sd = self.state_dict()
        w = lambda key: sd[key].reshape(sd[key].shape[0], -1)
        blob = _pack("pccx_pack_prob", _lib.load().pccx_prob_blob_floats(),
                     [w("model_pn.mlp_Modules.0.0.weight"), sd["model_pn.mlp_Modules.0.0.bias"],
                      w("model_pn.mlp_Modules.1.0.weight"), sd["model_pn.mlp_Modules.1.0.bias"],
                      w("model_pn.mlp_Modules.2.0.weight"), sd["model_pn.mlp_Modules.2.0.bias"],
                      w("model_mlp.0.weight"), sd["model_mlp.0.bias"], w("model_mlp.2.weight"), sd["model_mlp.2.bias"],
                      w("model_mlp.4.weight"), sd["model_mlp.4.bias"]], [self.d, self.L])
        self._blob = blob.to(device)
        return self

    def run(self, sampled_xyz, want=("pmf",), distinct=False, tiles=False):
        """sampled_xyz (B,S,3) -> dict with any of pmf (B,S,d,L), cdf (B,S,d,L+1), cdf_int (int32).
        distinct=True (clouds whose centres repeat, octree_mode "reference"): the fused kernel that evaluates each distinct centre of a
        cloud once, for S <= 64 -- the same outputs bit for bit; other shapes take the usual path.
        tiles=True (opt-in; few clouds of many centres, a whole room's 8192): pccx_prob_forward_tiled, the 16-centre tiles of every
        cloud dealt over the chip in three launches where the usual kernel gives a cloud to one workgroup -- the same outputs bit for
        bit, so `distinct` is ignored under it.  Shapes outside the fused kernel's take the generic layers either way."""
        x = _f32c(sampled_xyz, "ConditionalProbabilityModel")
        B, S, _ = x.shape
        if not self.fused_ok(S):
            return self._run_generic(x, want)
        if self._blob is None or self._blob.device != x.device:
            self.pack(x.device)
        r, ptrs = self._outputs(want, B, S, x.device)
        if tiles:
            ws = workspace("prob_tiled", max(int(_lib.load().pccx_prob_forward_tiled_workspace_floats(B, S)), 4), x.device)
            _lib.call("pccx_prob_forward_tiled", x.data_ptr(), B, S, self.d, self.L, self._blob.data_ptr(), *ptrs, ws.data_ptr(), _stream())
            return r
        fn = "pccx_prob_forward_distinct" if distinct and S <= 64 else "pccx_prob_forward"
        _lib.call(fn, x.data_ptr(), B, S, self.d, self.L, self._blob.data_ptr(), *ptrs, _stream())
        return r

    def run_segments(self, sampled_xyz, seg_idx, n_seg, G):
        """The integer CDF of the listed segments' rows only (region decode): sampled_xyz (S,3) or (1,S,3) the centres of ONE cloud,
        seg_idx (>= n_seg) i32 on the device, ascending segments of G patches, n_seg a host int -> cdf_int (n_seg*G, d, L+1) i32
        whose row r is row seg_idx[r // G] * G + r % G of run(...)["cdf_int"][0], bit for bit (the rows past S of a ragged last
        segment hold row S - 1's table and are not to be read).  pccx_prob_feature (pass 1 over up to 64 workgroups, pass 1b) then
        pccx_prob_rows; the fused kernel's shapes only (fused_ok(S)), anything else raises: the caller falls back to run()."""
        x = _f32c(sampled_xyz, "ConditionalProbabilityModel.run_segments").reshape(-1, 3)
        S, n_seg, G = x.shape[0], int(n_seg), int(G)
        if not self.fused_ok(S):
            raise _lib.PccxError(f"run_segments: the fused probability kernel does not cover d={self.d}, L={self.L}, S={S}")
        if G < 1 or not 0 <= n_seg <= -(-S // G) or seg_idx.dtype != torch.int32 or seg_idx.numel() < n_seg:
            raise ValueError(f"run_segments: n_seg={n_seg} segments of G={G} patches from an int32 list of {seg_idx.numel()} for S={S}")
        if self._blob is None or self._blob.device != x.device:
            self.pack(x.device)
        out = torch.empty(n_seg * G, self.d, self.L + 1, device=x.device, dtype=torch.int32)
        if n_seg == 0:
            return out
        lib = _lib.load()
        ws = workspace("prob_feature", int(lib.pccx_prob_feature_workspace_floats(S)) + 512, x.device)
        feature = ws[:512]                                   # the workspace's base is 16-byte aligned
        _lib.call("pccx_prob_feature", x.data_ptr(), S, self._blob.data_ptr(), ws[512:].data_ptr(), feature.data_ptr(), _stream())
        _lib.call("pccx_prob_rows", x.data_ptr(), S, self.d, self.L, self._blob.data_ptr(), feature.data_ptr(),
                  seg_idx.contiguous().data_ptr(), n_seg, G, out.data_ptr(), _stream())
        return out

    def _outputs(self, want, B, S, device):
        """The wanted ones of pmf / cdf / cdf_int, and the three pointers the kernels take (null for an output not wanted)."""
        kinds = {"pmf": (self.L, torch.float32), "cdf": (self.L + 1, torch.float32), "cdf_int": (self.L + 1, torch.int32)}
        r = {name: torch.empty(B, S, self.d, n, device=device, dtype=dt) for name, (n, dt) in kinds.items() if name in want}
        return r, [r[name].data_ptr() if name in r else None for name in kinds]

    def _run_generic(self, x, want):
        """AE.ConditionalProbabilityModel.forward (AE.py:107-123) + pmf_to_cdf + torchac's integer CDF through the generic layers,
        for --d / --L / S outside the fused kernel's shapes: model_pn (generic PointNet), the three 1x1 convolutions as generic
        layers on the (B*S, 259) rows, then pccx_softmax_cdf."""
        B, S, _ = x.shape
        feature = self.model_pn(x.transpose(1, 2).contiguous())                                    # AE.py:111-112  (B, 256)
        rows = torch.cat((x, feature[:, None, :].expand(B, S, feature.shape[1])), dim=2).reshape(B * S, -1)   # :113-115
        buf = torch.zeros(B * S, (rows.shape[1] + 3) // 4 * 4, device=x.device, dtype=torch.float32)           # 16-byte rows
        buf[:, :rows.shape[1]] = rows
        rows = buf[:, :rows.shape[1]]
        for layer in _lazy_layers(self, x.device, lambda dev: _folded_sequence(list(self.model_mlp), dev)):
            rows = layer(rows)                                                                     # :117  (B*S, d*L)
        r, ptrs = self._outputs(want, B, S, x.device)
        _lib.call("pccx_softmax_cdf", rows.contiguous().data_ptr(), B * S * self.d, self.L, *ptrs, _stream())   # :119-123
        return r

    def forward(self, sampled_xyz):
        return self.run(sampled_xyz, ("pmf",))["pmf"]


def range_cap(nsym):
    """Default output capacity per cloud of the range coder: 16-bit frequencies with every symbol's frequency >= 1 cost at
    most 16 bits per symbol, plus the flush."""
    return int(nsym) * 2 + 16


def _encoder_args(who, cdf_int, latent_q, L, out, nb, cap):
    """What the three encoders take from cdf_int (B,nsym,L+1) / latent_q (B,nsym) -> (B, nsym, q, out, nb): the f32 symbols and
    dense destinations, the caller's or new ones (out of cap(nsym) bytes per cloud)."""
    B = cdf_int.shape[0]
    nsym = cdf_int[0].numel() // (L + 1) if B else 0
    q = _f32c(latent_q.reshape(B, nsym), who)
    if out is None:
        out = torch.empty(B, cap(nsym), device=q.device, dtype=torch.uint8)
    if nb is None:
        nb = torch.empty(B, device=q.device, dtype=torch.int32)
    if (out.dim() != 2 or out.shape[0] != B or out.dtype != torch.uint8 or not out.is_contiguous() or tuple(nb.shape) != (B,)
            or nb.dtype != torch.int32 or not nb.is_contiguous()):
        raise _lib.PccxError(f"{who}: out must be dense (B,cap) u8 and nb dense (B,) i32")
    return B, nsym, q, out, nb


def _decoder_args(cdf_int, bytes_, nbytes, L, latent=True, status=False):
    """What the whole-batch decoders take from cdf_int (B,nsym,L+1) and the streams -> (B, nsym, dense bytes_, i32 nbytes,
    latent_q (B,nsym) f32 to fill or None, cleared status (B,) i32 or None)."""
    B = cdf_int.shape[0]
    nsym = cdf_int[0].numel() // (L + 1) if B else 0
    bytes_ = bytes_.contiguous()
    return (B, nsym, bytes_, nbytes.to(torch.int32).contiguous(),
            torch.empty(B, nsym, device=bytes_.device, dtype=torch.float32) if latent else None,
            torch.zeros(B, device=bytes_.device, dtype=torch.int32) if status else None)


def _list_decoder_args(cdf_int, bytes_, nbytes, seg_sym, seg_idx, n_list, status):
    """The same for the listed segments of ONE cloud -> (table pointer, flat bytes_, i32 nbytes, list pointer, compact latent_q
    (n_list*seg_sym,) f32, its pointer, status (1,) i32: the caller's or a cleared one).  Pointers are None for an empty list."""
    bytes_ = bytes_.contiguous().reshape(-1)
    q = torch.empty(n_list * seg_sym, device=bytes_.device, dtype=torch.float32)
    if status is None:
        status = torch.zeros(1, device=bytes_.device, dtype=torch.int32)
    return (cdf_int.contiguous().data_ptr() if n_list else None, bytes_, nbytes.to(torch.int32).contiguous(),
            seg_idx.contiguous().data_ptr() if n_list else None, q, q.data_ptr() if n_list else None, status)


def _status_error(who, st, table):
    """The PccxError for per-cloud status words ``st`` (a host sequence) explained by ``table``, or None when all are 0."""
    import numpy as np
    st = np.asarray(st).reshape(-1)
    if not st.any():
        return None
    return _lib.PccxError(f"{who}: " + "; ".join(
        f"clouds {[int(b) for b in (st == code).nonzero()[0]]}: {why}" for code, why in table.items() if (st == code).any()))


def _checked(who, q, status, table, check):
    """check=True: read the status once and raise what it says, else latent_q; check=False: (latent_q, status), no synchronisation."""
    if not check:
        return q, status
    err = _status_error(who, status.cpu().numpy(), table)
    if err is not None:
        raise err
    return q


def _host_check(fn_name, data, *ints):
    """One of the library's host-side format checks on a bytes-like object (no GPU call) -> its status word."""
    import ctypes
    data = bytes(data)
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    return int(getattr(_lib.load(), fn_name)(ctypes.addressof(buf), len(data), *(int(v) for v in ints)))


def range_encode(cdf_int, latent_q, L, cap=None, out=None, nb=None):
    """torchac.encode_float_cdf on device: cdf_int (B,nsym,L+1) int32, latent_q (B,nsym) -> (bytes (B,cap) u8, nbytes (B)).
    A cloud whose stream does not fit ``cap`` bytes comes back with a NEGATIVE nbytes; codec.Compressed.to_host() raises on it
    (unreachable with the default cap).  out / nb: caller-provided dense destinations."""
    B, nsym, q, out, nb = _encoder_args("range_encode", cdf_int, latent_q, L, out, nb, lambda n: cap or range_cap(n))
    _lib.call("pccx_range_encode", cdf_int.contiguous().data_ptr(), q.data_ptr(), B, nsym, int(L), out.data_ptr(), out.shape[1],
              nb.data_ptr(), _stream())
    return out, nb


def range_decode(cdf_int, bytes_, nbytes, L):
    """torchac.decode_float_cdf on device -> latent_q (B,nsym) f32 (already minus L//2)."""
    B, nsym, bytes_, nbytes, q, _ = _decoder_args(cdf_int, bytes_, nbytes, L)
    _lib.call("pccx_range_decode", cdf_int.contiguous().data_ptr(), bytes_.data_ptr(), bytes_.shape[1], nbytes.data_ptr(), B, nsym, int(L),
              q.data_ptr(), _stream())
    return q


def _nsym_of(nsym_of, B, device):
    t = nsym_of if isinstance(nsym_of, torch.Tensor) else torch.as_tensor(list(nsym_of), dtype=torch.int32)
    t = t.to(device=device, dtype=torch.int32).contiguous()
    if tuple(t.shape) != (B,):
        raise _lib.PccxError(f"nsym_of: one int per cloud is expected, got {tuple(t.shape)} for {B} clouds")
    return t


def range_encode_n(cdf_int, latent_q, nsym_of, L, cap=None, out=None, nb=None):
    """range_encode for a ragged batch (pccx_range_encode_n): the rows of cdf_int (B,nsym,L+1) / latent_q (B,nsym) are nsym symbols
    apart and cloud b codes its first nsym_of[b] (a (B,) sequence or int32 tensor).  The bytes of cloud b are range_encode's on its
    own rows alone."""
    B, nsym, q, out, nb = _encoder_args("range_encode_n", cdf_int, latent_q, L, out, nb, lambda n: cap or range_cap(n))
    _lib.call("pccx_range_encode_n", cdf_int.contiguous().data_ptr(), q.data_ptr(), B, nsym, _nsym_of(nsym_of, B, q.device).data_ptr(), int(L),
              out.data_ptr(), out.shape[1], nb.data_ptr(), _stream())
    return out, nb


def range_decode_n(cdf_int, bytes_, nbytes, nsym_of, L):
    """range_decode for a ragged batch (pccx_range_decode_n) -> latent_q (B,nsym) f32: cloud b's first nsym_of[b] symbols, zeros
    behind them.  Foreign bytes are taken as range_decode takes them: nbytes cut to the row, bits past the stream read as zero."""
    B, nsym, bytes_, nbytes, q, _ = _decoder_args(cdf_int, bytes_, nbytes, L)
    _lib.call("pccx_range_decode_n", cdf_int.contiguous().data_ptr(), bytes_.data_ptr(), bytes_.shape[1], nbytes.data_ptr(), B, nsym,
              _nsym_of(nsym_of, B, bytes_.device).data_ptr(), int(L), q.data_ptr(), _stream())
    return q


# ---- split form of the latent stream (include/pccx.h: "PXS1" | nsym | seg_sym | 0 | len[P] | segments) -------------------------

SPLIT_HEADER = 12
SPLIT_MAX_SEGMENTS = 8192
SPLIT_STATUS = {1: "shorter than its header, or no 'PXS1' magic (written without a split, or not a .p.bin)",
                2: "nsym / seg_sym / reserved field disagree with the call (written with another split or another S)",
                3: "a segment length above its capacity, or header + segment lengths != the byte count (truncated or extended)"}


def split_segments(nsym, seg_sym):
    return -(-int(nsym) // int(seg_sym))


def split_cap(nsym, seg_sym):
    """Capacity per cloud of the split stream: the 12 fixed bytes, P lengths, P segments of range_cap(seg_sym)."""
    P = split_segments(nsym, seg_sym)
    return SPLIT_HEADER + 2 * P + P * range_cap(seg_sym)


def split_max_seg_sym(L):
    """The largest seg_sym the split entry points take at L levels (the LDS image of one segment, both directions); 0 for an L
    outside 2..63."""
    return int(_lib.load().pccx_range_split_max_seg_sym(int(L)))


def _split_workspace(B, nsym, seg_sym, device):
    need = int(_lib.load().pccx_range_split_workspace_bytes(int(B), int(nsym), int(seg_sym)))
    return workspace("range_split", max(need // 4, 4), device)


def range_encode_split(cdf_int, latent_q, L, seg_sym, out=None, nb=None):
    """The split stream of every cloud: cdf_int (B,nsym,L+1) int32, latent_q (B,nsym) -> (bytes (B,cap) u8, nbytes (B)); segment p
    codes symbols [p*seg_sym, (p+1)*seg_sym) as range_encode codes a stream of that length.  nbytes < 0: `cap` too small, as there."""
    seg_sym = int(seg_sym)
    B, nsym, q, out, nb = _encoder_args("range_encode_split", cdf_int, latent_q, L, out, nb, lambda n: split_cap(n, max(seg_sym, 1)))
    ws = _split_workspace(B, nsym, seg_sym, q.device)
    _lib.call("pccx_range_encode_split", cdf_int.contiguous().data_ptr(), q.data_ptr(), B, nsym, seg_sym, int(L), out.data_ptr(),
              out.shape[1], nb.data_ptr(), ws.data_ptr(), _stream())
    return out, nb


def range_decode_split(cdf_int, bytes_, nbytes, L, seg_sym, check=True):
    """The inverse -> latent_q (B,nsym) f32.  check=True reads the per-cloud status once and raises PccxError naming the clouds whose
    header is refused (SPLIT_STATUS); check=False returns (latent_q, status (B,) i32 on the device) without a synchronisation -- a
    refused cloud's symbols are those of an empty stream."""
    seg_sym = int(seg_sym)
    B, nsym, bytes_, nbytes, q, status = _decoder_args(cdf_int, bytes_, nbytes, L, status=True)
    ws = _split_workspace(B, nsym, seg_sym, bytes_.device)
    _lib.call("pccx_range_decode_split", cdf_int.contiguous().data_ptr(), bytes_.data_ptr(), bytes_.shape[1], nbytes.data_ptr(), B, nsym,
              seg_sym, int(L), q.data_ptr(), status.data_ptr(), ws.data_ptr(), _stream())
    return _checked("range_decode_split", q, status, SPLIT_STATUS, check)


def split_status_error(who, st):
    """The PccxError range_decode_split raises for per-cloud status words ``st`` (a host sequence), or None when all are 0."""
    return _status_error(who, st, SPLIT_STATUS)


def range_decode_split_list(cdf_int, bytes_, nbytes, L, seg_sym, nsym, seg_idx, n_list, status=None):
    """range_decode_split for the listed segments of ONE cloud: cdf_int (n_list*seg_sym, L+1) i32 compact table rows (segment j of
    the list at rows j*seg_sym ...), bytes_ (cap,) or (1,cap) u8 the cloud's file, nbytes (1,) i32, nsym the cloud's symbol count,
    seg_idx i32 on the device (the first n_list entries, ascending segment numbers), n_list a host int ->
    (latent_q (n_list*seg_sym,) f32 compact, status (1,) i32 on the device, as range_decode_split(check=False) gives it).  No byte of
    an unlisted segment is read.  n_list = 0 runs the header check alone.  status: an int32 device tensor to write instead of a new one."""
    n_list, seg_sym, nsym = int(n_list), int(seg_sym), int(nsym)
    cdf_p, bytes_, nbytes, idx_p, q, q_p, status = _list_decoder_args(cdf_int, bytes_, nbytes, seg_sym, seg_idx, n_list, status)
    ws = _split_workspace(1, nsym, seg_sym, bytes_.device)
    _lib.call("pccx_range_decode_split_list", cdf_p, bytes_.data_ptr(), bytes_.numel(), nbytes.data_ptr(), nsym, seg_sym, int(L), idx_p,
              n_list, q_p, status.data_ptr(), ws.data_ptr(), _stream())
    return q, status


def split_stream_status(data, nsym, seg_sym):
    """pccx_split_stream_check_host on a bytes-like object (no GPU call): 0, or a key of SPLIT_STATUS."""
    return _host_check("pccx_split_stream_check_host", data, nsym, seg_sym, range_cap(seg_sym))


# ---- entry-point index of the single stream (include/pccx.h: "PXI1" | nsym | seg_sym | P | {low, high, pos}[P]) -----------------
# The .p.bin stays range_encode's bytes; the sidecar lets one wave per segment enter it.  Limits are the split path's.

INDEX_HEADER = 16
INDEX_ENTRY = 12
INDEX_STATUS = {1: "shorter than its header, no 'PXI1' magic, or not 16 + 12*P bytes (truncated, or not a .p.idx)",
                2: "nsym / seg_sym / P field disagree with the call (written with another p_index or another S)",
                3: "an entry's position lies below the one before it",
                4: "an entry's position lies beyond the stream's last bit (the index of another .p.bin)",
                5: "consecutive positions further apart than the bits a segment may take",
                6: "an entry's interval is no state of the coder, or entry 0 is not the initial state"}


def index_bytes(nsym, seg_sym):
    """Bytes of one cloud's sidecar: 16 + 12 * ceil(nsym / seg_sym)."""
    return INDEX_HEADER + INDEX_ENTRY * split_segments(nsym, seg_sym)


def _index_workspace(B, nsym, seg_sym, device):
    need = int(_lib.load().pccx_range_index_workspace_bytes(int(B), int(nsym), int(seg_sym)))
    return workspace("range_index", max(need // 4, 4), device)


def _index_rows(index, B, who):
    """A sidecar tensor as dense (B, idx_stride) u8 rows on the device."""
    if index.dtype != torch.uint8 or index.dim() not in (1, 2):
        raise _lib.PccxError(f"{who}: index must be (B, bytes) or (bytes,) u8")
    index = index.reshape(B, -1).contiguous()
    return index


def range_encode_indexed(cdf_int, latent_q, L, seg_sym, cap=None, out=None, nb=None):
    """range_encode that also writes the entry-point index: -> (bytes (B,cap) u8, nbytes (B), index (B, index_bytes(nsym, seg_sym)) u8).
    The bytes and counts are range_encode's; index row b is the file <name>.p.idx of cloud b."""
    seg_sym = int(seg_sym)
    B, nsym, q, out, nb = _encoder_args("range_encode_indexed", cdf_int, latent_q, L, out, nb, lambda n: cap or range_cap(n))
    index = torch.empty(B, index_bytes(nsym, max(seg_sym, 1)), device=q.device, dtype=torch.uint8)
    _lib.call("pccx_range_encode_indexed", cdf_int.contiguous().data_ptr(), q.data_ptr(), B, nsym, seg_sym, int(L), out.data_ptr(),
              out.shape[1], nb.data_ptr(), index.data_ptr(), _stream())
    return out, nb, index


def range_index_build(cdf_int, bytes_, nbytes, L, seg_sym, return_latent=False):
    """The index of existing streams (files written without one, the reference's included): the sequential decoder run once ->
    index (B, index_bytes) u8, bit for bit what range_encode_indexed writes for the same stream; with return_latent also the
    symbols it decoded on the way, (index, latent_q (B,nsym) f32)."""
    seg_sym = int(seg_sym)
    B, nsym, bytes_, nbytes, q, _ = _decoder_args(cdf_int, bytes_, nbytes, L, latent=return_latent)
    index = torch.empty(B, index_bytes(nsym, max(seg_sym, 1)), device=bytes_.device, dtype=torch.uint8)
    _lib.call("pccx_range_index_build", cdf_int.contiguous().data_ptr(), bytes_.data_ptr(), bytes_.shape[1], nbytes.data_ptr(), B, nsym,
              seg_sym, int(L), index.data_ptr(), q.data_ptr() if return_latent else None, _stream())
    return (index, q) if return_latent else index


def range_decode_indexed(cdf_int, bytes_, nbytes, index, L, seg_sym, index_nbytes=None, check=True):
    """range_decode by one wave per segment of seg_sym symbols, each entering the ONE stream at its entry of `index` (B, bytes) u8 ->
    latent_q (B,nsym) f32, equal to range_decode's.  index_nbytes: (B) i32 byte counts of the sidecars where they may be shorter
    than their rows (files).  check=True reads the per-cloud status once and raises PccxError naming the clouds whose sidecar is
    refused (INDEX_STATUS); check=False returns (latent_q, status (B,) i32 on the device) without a synchronisation -- a refused
    cloud's symbols are those of empty segments."""
    seg_sym = int(seg_sym)
    index = _index_rows(index, cdf_int.shape[0], "range_decode_indexed")
    B, nsym, bytes_, nbytes, q, status = _decoder_args(cdf_int, bytes_, nbytes, L, status=True)
    if index_nbytes is not None:
        index_nbytes = index_nbytes.to(torch.int32).contiguous()
    ws = _index_workspace(B, nsym, seg_sym, bytes_.device)
    _lib.call("pccx_range_decode_indexed", cdf_int.contiguous().data_ptr(), bytes_.data_ptr(), bytes_.shape[1], nbytes.data_ptr(),
              index.data_ptr(), index.shape[1], index_nbytes.data_ptr() if index_nbytes is not None else None, B, nsym, seg_sym, int(L),
              q.data_ptr(), status.data_ptr(), ws.data_ptr(), _stream())
    return _checked("range_decode_indexed", q, status, INDEX_STATUS, check)


def index_status_error(who, st):
    """The PccxError range_decode_indexed raises for per-cloud status words ``st`` (a host sequence), or None when all are 0."""
    return _status_error(who, st, INDEX_STATUS)


def range_decode_indexed_list(cdf_int, bytes_, nbytes, index, L, seg_sym, nsym, seg_idx, n_list, status=None):
    """range_decode_indexed for the listed segments of ONE cloud, the counterpart of range_decode_split_list: cdf_int
    (n_list*seg_sym, L+1) i32 compact table rows, bytes_ the cloud's .p.bin, nbytes (1,) i32, index the idx bytes of its sidecar
    (a 1-d u8 tensor: its length is the sidecar's), seg_idx i32 on the device, n_list a host int -> (latent_q (n_list*seg_sym,) f32
    compact, status (1,) i32 on the device).  Only the bytes of the listed segments' spans are read.  n_list = 0 runs the check alone."""
    index = index.contiguous().reshape(-1)
    if index.dtype != torch.uint8:
        raise _lib.PccxError("range_decode_indexed_list: index must be u8")
    n_list, seg_sym, nsym = int(n_list), int(seg_sym), int(nsym)
    cdf_p, bytes_, nbytes, idx_p, q, q_p, status = _list_decoder_args(cdf_int, bytes_, nbytes, seg_sym, seg_idx, n_list, status)
    ws = _index_workspace(1, nsym, seg_sym, bytes_.device)
    _lib.call("pccx_range_decode_indexed_list", cdf_p, bytes_.data_ptr(), bytes_.numel(), nbytes.data_ptr(), index.data_ptr(),
              index.numel(), nsym, seg_sym, int(L), idx_p, n_list, q_p, status.data_ptr(), ws.data_ptr(), _stream())
    return q, status


def index_status(data, stream_bytes, nsym, seg_sym):
    """pccx_entry_index_check_host on a bytes-like sidecar for a .p.bin of stream_bytes bytes (no GPU call): 0, or a key of INDEX_STATUS."""
    return _host_check("pccx_entry_index_check_host", data, stream_bytes, nsym, seg_sym)
