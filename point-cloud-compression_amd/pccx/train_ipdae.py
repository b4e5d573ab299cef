"""The training step of train.py:156-245 (``--model AE``: the IPDAE autoencoder of AE.py with its ConditionalProbabilityModel) on libpccx.so.

    batch_x, center, longest = pn_kit.normalize(batch_x, margin=0.01)                         # :171
    sampled_xyz = index_points(batch_x, farthest_point_sample_batch(batch_x, S))              # :178
    octree_codes, sampled_bits = encode_sampled_np(sampled_xyz, 1, N, OCTREE_BPP_DICT[K])     # :183
    rec_sampled_xyz = decode_sampled_np(octree_codes, 1)                                       # :184 (octree_np.decode, bug-compatible)
    x_patches = (knn_points(rec_sampled_xyz, batch_x, K) - rec_sampled_xyz) * (N / N0) ** (1/3)   # :192-199
    patches_pred, bottleneck, latent_quantized = ae(x_patches)                                 # :200 (AE.py:34-55)
    pmf = prob(rec_sampled_xyz); feature_bits = estimate_bits_from_pmf(pmf, sym) / (B * N)    # :204-208
    loss = chamfer_distance(pc_pred, batch_x) + lambda * feature_bits / (B * N)                # :211-222 (AE.py:61-70)
    loss.backward(); optimizer.step()                                                          # :229-230 (Adam over ae + prob)

Every step of the selection (normalize, FPS, octree depth search / encode / decode, kNN patches, in-patch 16-NN) is the codec's own HIP
kernel; the two networks are evaluated layer by layer through the autograd Functions of pccx.train (each a pair of HIP launches behind
the C ABI: pccx_linear / pccx_linear_dw / pccx_group_max_arg / pccx_chamfer_grad ...), so torch.autograd only sequences the backward;
Adam is pccx.train.Adam (two launches over all tensors).  The models are pccx.models.AE / ConditionalProbabilityModel: their parameters
are the reference's state_dict, and the checkpoints this trainer writes load into the codec (compress.py:58) unchanged.
fp32 by default (the reference's CPU branch, contextlib.nullcontext at :175); autocast=True is the bf16 form of pccx.train.
AE.py has no BatchNorm on this path (bn=False at AE.py:16-27).  ``--model PPPF-AE`` (train-mode BatchNorm over GROUPED rows) is not built.
octree_mode="full" (select_patches, forward_loss, IpdaeTrainer; train.py --octree-mode full) replaces :184 by the intended decode and
normalises every cloud by its own box: the trainer then selects, bit for bit, the patches ``compress.py --octree-mode full`` codes, for
any S = N * ALPHA / K up to 1024 (clouds above 32768 points through the grid's wide-K walk, as the codec), and IpdaeTrainer.validate runs the current weights through that codec.
Clouds of different sizes in one step (train.py --ragged; "full" mode only): select_patches_ragged, forward_loss_ragged,
IpdaeTrainer.step_ragged / graphed_ragged / validate_ragged, the trainer's side of Codec.compress_ragged.
Files of any size (train.py --crop): CropSampler cuts every step's batch as nearest-n crops of a store of clouds.
"""
import torch

from . import _lib, ops, train
from .codec import KNN_BRUTE_MAX_N
from .train import GroupMaxFn, LinearFn, ReluFn

OCTREE_BPP_DICT = {1024: 0.07, 512: 0.125, 256: 0.25, 128: 0.5, 64: 1.0}      # pn_kit.py:17-23


class LinearReluFn(torch.autograd.Function):
    """relu(x W^T + b) as ONE launch (pccx_linear with its ReLU epilogue) whose backward masks dY with the saved output: the separate
    ReLU pass of pccx.train (z written, read back, y written) was a third of this step's activation traffic -- 64 patches x 256 points x
    16 neighbours = 262 144 rows through the set-abstraction stack.  Same values as LinearFn + ReluFn."""

    @staticmethod
    def forward(ctx, x, W, b):
        x = x.contiguous()
        W2 = W.reshape(W.shape[0], -1).contiguous()
        N, K = W2.shape
        ctx.flags = 2 if train._AUTOCAST else 0
        ctx.det = train._DETERMINISTIC
        y = train._linear_raw(x, train._packed(W2, False), b, N, K, ctx.flags | 1)
        ctx.save_for_backward(x, W2, y)
        ctx.has_bias, ctx.wshape = b is not None, W.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W2, y = ctx.saved_tensors
        N, K = W2.shape
        M = x.shape[0]
        dz = torch.empty_like(y)
        _lib.call("pccx_relu_backward", dy.contiguous().data_ptr(), y.data_ptr(), y.numel(), dz.data_ptr(), train._stream())
        dx = train._linear_raw(dz, train._packed(W2, True), None, K, N, ctx.flags) if ctx.needs_input_grad[0] else None
        dW = train._dw(dz, x, M, N, K, N, x.stride(0), ctx.flags, ctx.det)
        db = train._bias_grad(dz, M, N, ctx.det) if ctx.has_bias else None
        return dx, dW.view(ctx.wshape), db


def _lin(x, conv, relu):
    N_, K_ = conv.weight.shape[0], conv.weight[0].numel()
    if relu and x.shape[0] > 8 and not train._is_wide(x.shape[0], N_, K_):    # (a few rows: pccx.train's skinny / role-swapped layers)
        return LinearReluFn.apply(x, conv.weight, conv.bias)
    y = LinearFn.apply(x, conv.weight, conv.bias)
    return ReluFn.apply(y) if relu else y


def inpatch_neighbour_rows(x, nk):
    """pn_kit.py:190-191 with S == N: for every point of every patch its nk nearest neighbours inside the patch, relative to the point ->
    rows (P * K * nk, 3).  nk = 16 (AE.py:16) takes the codec's own selection kernel (pccx_patch_knn16: a byte per index; the SET of
    pytorch3d's knn_points -- the order inside a group does not matter to the max-pool that follows) and a gather."""
    P, K, _ = x.shape
    if nk == 16 and K % 16 == 0 and 16 <= K <= 1024:
        lib = _lib.load()
        ib = int(lib.pccx_patch_knn16_index_bytes(K))
        tab = torch.empty(int(lib.pccx_patch_knn16_bytes(P, K)), device=x.device, dtype=torch.uint8)
        _lib.call("pccx_patch_knn16", x.data_ptr(), P, K, tab.data_ptr(), train._stream())
        idx = tab.view(P, K, 16).to(torch.int64) if ib == 1 else (tab.view(torch.int16).view(P, K, 16).to(torch.int64) & 0xFFFF)
        return (ops.index_points(x, idx) - x.view(P, K, 1, 3)).reshape(P * K * 16, 3).contiguous()
    return ops.knn_points(x, x, nk, patch_scale=1.0).knn.reshape(P * K * nk, 3).contiguous()


def ae_forward_train(ae, x_patches):
    """AE.forward (AE.py:34-55) recording a graph: x_patches (P, K, 3) -> (new_xyz (P, k, 3), latent (P, d), latent_quantized (P, d))."""
    P, K, _ = x_patches.shape
    sa, pn = ae.sa, ae.pn
    if sa.npoint != K:
        raise _lib.PccxError(f"train_ipdae: AE was built for K={sa.npoint}, patches have {K} points")
    x = x_patches.detach().contiguous()
    with torch.no_grad():
        rows = inpatch_neighbour_rows(x, sa.K)                                        # pn_kit.py:190-191
    h = _lin(rows, sa.conv0, True)                                                    # :198
    h = _lin(h, sa.conv1, True)                                                       # :199
    h = _lin(h, sa.conv2, sa.finalRelu)                                               # :201-205
    feat = GroupMaxFn.apply(h.view(P * K, sa.K, -1))                                  # :207 max over the 16 neighbours
    h = torch.cat([x.reshape(P * K, 3), feat], dim=1)                                 # AE.py:39 (xyz first)
    for m in pn.mlp_Modules:
        h = _lin(h, m[0], len(m) > 1)                                                 # pn_kit.py:138-139
    z = GroupMaxFn.apply(h.view(P, K, -1))                                            # :141 max over the patch's points
    spread = ae.L - 0.2                                                               # AE.py:43
    latent = torch.sigmoid(z) * spread - spread / 2                                   # :44
    q = ops.ste_round(latent)                                                         # :45 (round, straight-through gradient)
    h = q
    lins = [m for m in ae.inv_pool if isinstance(m, torch.nn.Linear)]
    for m in lins:
        h = _lin(h, m, True)                                                          # :19-26: ReLU after each of the three
    k = ae.k
    lo = h.view(P, -1, k).permute(0, 2, 1).reshape(P * k, -1)                         # :49 view(BS, -1, k), as rows per output point
    h = torch.cat([lo, q[:, None, :].expand(P, k, q.shape[1]).reshape(P * k, -1)], dim=1)   # :50-51 (linear output first)
    for m in ae.inv_mlp.mlp_Modules:
        h = _lin(h, m[0], len(m) > 1)                                                 # :52
    return h.view(P, k, 3), latent, q


def prob_forward_train(prob, sampled_xyz):
    """ConditionalProbabilityModel.forward (AE.py:107-123) recording a graph: (B, S, 3) -> pmf (B, S, d, L)."""
    B, S, _ = sampled_xyz.shape
    rows = sampled_xyz.detach().reshape(B * S, 3).contiguous()
    h = rows
    for m in prob.model_pn.mlp_Modules:
        h = _lin(h, m[0], len(m) > 1)
    feat = GroupMaxFn.apply(h.view(B, S, -1))                                         # :112 (B, 256)
    h = torch.cat([rows, feat[:, None, :].expand(B, S, feat.shape[1]).reshape(B * S, -1)], dim=1)   # :115 (xyz first)
    convs = [m for m in prob.model_mlp if isinstance(m, torch.nn.Conv2d)]
    for i, m in enumerate(convs):
        h = _lin(h, m, i + 1 < len(convs))                                            # :117
    return torch.softmax(h.view(B, S, prob.d, prob.L), dim=3)                         # :118-120


def estimate_bits_from_pmf(pmf, sym):
    """pn_kit.estimate_bits_from_pmf (pn_kit.py:439-450)"""
    L = pmf.shape[-1]
    p = torch.gather(pmf.reshape(-1, L), 1, sym.reshape(-1, 1))
    return torch.sum(-torch.log2(p.clamp(min=1e-3)))


OCTREE_MODES = ("reference", "full")                                           # the spelling of compress.py / decompress.py --octree-mode


def check_selection(S, K, octree_mode="reference"):
    """The limits of select_patches, on the host and before any launch: ValueError for an unknown mode, PccxError naming the limit."""
    if octree_mode not in OCTREE_MODES:
        raise ValueError(f"train_ipdae: octree_mode must be one of {OCTREE_MODES}, got {octree_mode!r}")
    if octree_mode == "reference" and S != 64:
        raise _lib.PccxError(f"train_ipdae: octree_np.decode returns 64 centres whatever it is given (octree_np.py:100-111); S = N * ALPHA / K "
                             f"must be 64 (got {S})")
    if not 1 <= S <= ops.PATCH_GROUPS_MAX_S:
        raise _lib.PccxError(f"train_ipdae: octree_mode='full' trains on S = N * ALPHA / K patches in 1..{ops.PATCH_GROUPS_MAX_S} (the narrow octree "
                             f"coder and decode and the one-workgroup FPS, which a captured step can hold), got S = {S}")
    if K not in OCTREE_BPP_DICT:
        raise _lib.PccxError(f"train_ipdae: --K must be one of {sorted(OCTREE_BPP_DICT)} (pn_kit.py:17-23), got {K}")


def select_patches(batch_x, S, K, N, N0, starts, octree_mode="reference"):
    """train.py:171-199 -- everything in front of the networks: depends on the data and the FPS start indices only.
    -> (batch_x normalised (B,N,3), rec_sampled_xyz (B,S,3), x_patches (B*S,K,3) scaled, sampled_bits (device scalar), scale)
    Nothing here reads a result on the host: the whole step can be captured into a hipGraph (GraphedIpdaeStep).
    octree_mode="full": the centres are the level-by-level decode of the octree stream, the ones ``compress.py --octree-mode full``
    centres its patches on, S anywhere in 1..ops.PATCH_GROUPS_MAX_S, and every cloud is normalised by its own box.  x, rec and patches are
    then bit for bit the pcn, rec_sampled and patches of Codec(octree_mode="full", group_duplicates=False).compress(keep_extras=True)."""
    B = batch_x.shape[0]
    check_selection(S, K, octree_mode)
    if octree_mode == "full":
        x, _, _ = ops.normalize(batch_x, margin=0.01)                                 # compress.py:90, one box per cloud as Codec.compress
    else:
        # :171 -- pn_kit.normalize reads the centre and the longest side from pc[0] ONLY (pn_kit.py:50-53: "one point cloud"; train.py:40
        # says the batch size must be 1) and applies them to whatever it is given: a batch is normalised by its FIRST cloud's box.  Reproduced.
        x, c0, l0 = ops.normalize(batch_x[:1].contiguous(), margin=0.01)
        if B > 1:
            rest = ((batch_x[1:].float() - c0.view(1, 1, 3)) * (1 - 0.01)) / l0.view(1, 1, 1) + 0.5       # pn_kit.py:55-57, op for op
            x = torch.cat([x, rest], dim=0).contiguous()
    sampled = ops.index_points(x, ops.farthest_point_sample_batch(x, S, starts))      # :178
    enc = ops.octree_encode(sampled, N, OCTREE_BPP_DICT[K])                           # :183
    rec, _ = ops.octree_decode(enc["bytes"], enc["nbytes"], octree_mode, S)           # :184 as written ("reference") or as intended ("full")
    sampled_bits = enc["nbits"].sum()                                                 # codebits: the streams' lengths in bits (device scalar)
    scale = float((N / N0) ** (1 / 3))
    # :192-199.  The all-pairs kernels keep a cloud's keys in LDS and stop at KNN_BRUTE_MAX_N = 32768 points; above it (K >= 128 at the
    # larger S of "full" mode) the grid's wide-K walk finds the same patches bit for bit, by Codec.compress's own rule (knn_search="auto").
    # Both are stream-ordered launches without a read-back, so the captured step holds either.
    patches = ops.knn_points(rec, x, K, patch_scale=scale, search="grid" if x.shape[1] > KNN_BRUTE_MAX_N else None).knn.view(B * S, K, 3)
    return x, rec, patches, sampled_bits, scale


def forward_loss(ae, prob, batch_x, starts, lam, S, K, N, N0, octree_mode="reference"):
    """the forward of train.py:171-222 -> (loss, fbpp, bpp) with the graph of loss recorded; octree_mode as select_patches takes it (the
    loss arithmetic is the same in both modes)"""
    B = batch_x.shape[0]
    x, rec, patches, sampled_bits, scale = select_patches(batch_x, S, K, N, N0, starts, octree_mode)
    patches_pred, _, q = ae_forward_train(ae, patches)                                # :200
    patches_pred = patches_pred / scale                                               # :201
    pmf = prob_forward_train(prob, rec)                                               # :204
    sym = (q.detach().view(B, S, ae.d) + ae.L // 2).long().clamp(0, ae.L - 1)         # :205-206
    feature_bits = estimate_bits_from_pmf(pmf, sym) / (B * N)                         # :208
    bpp = (sampled_bits + feature_bits) / (B * N)                                     # :211
    fbpp = feature_bits / (B * N)                                                     # :212
    pc_pred = (patches_pred.view(B, S, -1, 3) + rec.view(B, S, 1, 3)).reshape(B, -1, 3)    # :214-216
    d, _ = ops.chamfer_distance(pc_pred, x)                                           # AE.py:67
    return d + lam * fbpp, fbpp, bpp                                                  # AE.py:68-70


def select_patches_ragged(pc, n_dev, S_dev, scale_dev, S_cap, K, starts):
    """select_patches(octree_mode="full") for clouds of different sizes in one launch sequence: pc (B, N_cap, 3) with cloud b in its
    first n[b] rows (the rows behind them reach no result), cloud b sampling S[b] <= S_cap centres and scaling its patches by scale[b].
    It is the selection of Codec.compress_ragged without the duplicate table: every one of the B * S_cap patches is searched, and
    the patches behind S[b] -- centred on repeats of the cloud's last decoded centre -- are copies of its last real one.
    -> (x normalised (B,N_cap,3), zeros behind n[b]; rec (B,S_cap,3); patches (B*S_cap,K,3); nbits (B,) int32: the octree stream of
    every cloud in bits, not their sum).  For every cloud x, the first S[b] centres and the first S[b] patches are bit for bit the pcn,
    rec_sampled and patches of Codec(octree_mode="full").compress_ragged(keep_extras=True).
    n_dev, S_dev (B,) int32, scale_dev (B,) float32 and starts (B,) int32 are device buffers: nothing is read back, and a captured
    step (RaggedGraphedIpdaeStep) changes them between replays."""
    B = pc.shape[0]
    x, _, _ = ops.normalize_n(pc, n_dev, margin=0.01)
    sampled = ops.index_points(x, ops.farthest_point_sample_n(x, n_dev, S_cap, S_dev, starts))
    enc = ops.octree_encode_n(sampled, S_dev, n_dev, OCTREE_BPP_DICT[K])
    rec, _ = ops.octree_decode(enc["bytes"], enc["nbytes"], "full", S_cap)            # the centres past S[b] repeat the last one
    patches = ops.knn_points_n(rec, x, n_dev, K, scale_dev).knn.view(B * S_cap, K, 3)
    return x, rec, patches, enc["nbits"]


def forward_loss_ragged(ae, prob, pc, n_dev, S_dev, scale_dev, starts, lam, S_cap, K):
    """forward_loss(octree_mode="full") over a ragged batch -> (loss, fbpp, bpp) with the graph of loss recorded.

    The networks run on all B * S_cap patches through ae_forward_train / prob_forward_train unchanged: there is no BatchNorm on this
    path, a padded patch is a copy of its cloud's last real one, and the probability model's group max over repeats of the last centre
    is the max over the real ones.  Cloud b's prediction is its first S[b] * k rows; with n_b points, S_b patches and nbits_b octree bits
      chamfer_b = mean_{i < S_b k} min_j |pred_i - x_j|^2 + mean_{j < n_b} min_i |pred_i - x_j|^2      (ops.chamfer_distance by length)
      bits_b    = sum_{s < S_b} sum_c -log2 clamp(pmf[b, s, c, sym], 1e-3)                            (padded patches masked out)
      fb_b = bits_b / n_b,   fbpp_b = fb_b / n_b,   bpp_b = (nbits_b + fb_b) / n_b
      loss = mean_b chamfer_b + lam * mean_b fbpp_b;   reported fbpp = mean_b fbpp_b, bpp = mean_b bpp_b
    that is the mean over the clouds of what forward_loss computes for each cloud alone at B = 1.  It keeps the double division of
    train.py:208-212, so a one-cloud ragged step is the dense step.  For B > 1 clouds of equal size the rate term is B times the dense
    step's: that one divides by B * N twice, inherited from a script that says its batch size must be 1 (train.py:40)."""
    B = pc.shape[0]
    x, rec, patches, nbits = select_patches_ragged(pc, n_dev, S_dev, scale_dev, S_cap, K, starts)
    patches_pred, _, q = ae_forward_train(ae, patches)                                # :200
    patches_pred = patches_pred.view(B, S_cap, -1, 3) / scale_dev.view(B, 1, 1, 1)    # :201, every cloud by its own scale
    pmf = prob_forward_train(prob, rec)                                               # :204
    sym = (q.detach().view(B, S_cap, ae.d) + ae.L // 2).long().clamp(0, ae.L - 1)     # :205-206
    p = torch.gather(pmf.reshape(-1, ae.L), 1, sym.reshape(-1, 1)).view(B, S_cap, ae.d)
    real = torch.arange(S_cap, device=pc.device, dtype=torch.int32).view(1, S_cap) < S_dev.view(B, 1)
    bits = ((-torch.log2(p.clamp(min=1e-3))).sum(dim=2) * real).sum(dim=1)            # pn_kit.py:439-450 over the cloud's own patches
    nf = n_dev.to(torch.float32)
    fb = bits / nf                                                                    # :208
    bpp = ((nbits.to(torch.float32) + fb) / nf).mean()                                # :211
    fbpp = (fb / nf).mean()                                                           # :212
    pc_pred = (patches_pred + rec.view(B, S_cap, 1, 3)).reshape(B, -1, 3)             # :214-216
    d, _ = ops.chamfer_distance(pc_pred, x, x_lengths=S_dev * int(ae.k), y_lengths=n_dev)
    return d + lam * fbpp, fbpp, bpp


class IpdaeTrainer:
    """The state of train.py's loop for ``--model AE``: the two models, Adam over both (train.py:131-134), the step counter with the
    rate term switched on at rate_loss_enable_step (:218-221) and the learning-rate decay (:250-254)."""

    def __init__(self, ae, prob, N=8192, N0=1024, ALPHA=2, K=256, lr=0.0005, lamda=1e-6, rate_loss_enable_step=40000, lr_decay=0.1,
                 lr_decay_steps=60000, autocast=False, deterministic=False, octree_mode="reference"):
        self.ae, self.prob = ae, prob
        self.N, self.N0, self.K, self.S = int(N), int(N0), int(K), int(N) * int(ALPHA) // int(K)
        self.ALPHA = int(ALPHA)
        if octree_mode != "reference":                                # "reference" keeps refusing at its first step, as before
            check_selection(self.S, self.K, octree_mode)
        self.octree_mode = octree_mode
        self.lamda, self.rate_loss_enable_step = float(lamda), int(rate_loss_enable_step)
        self.lr, self.lr_decay, self.lr_decay_steps = float(lr), float(lr_decay), int(lr_decay_steps)
        self.autocast, self.deterministic = bool(autocast), bool(deterministic)
        self.opt = train.Adam(list(ae.parameters()) + list(prob.parameters()), lr=self.lr)
        self.global_step = 0

    def step(self, batch_x, starts):
        """one iteration (train.py:162-254) -> dict(loss, fbpp, bpp) of python floats; starts: the FPS start index per cloud (:178 draws it
        with torch.randint inside farthest_point_sample_batch, pn_kit.py:321)"""
        if batch_x.dim() != 3 or batch_x.shape[1] != self.N or batch_x.shape[2] != 3:
            raise _lib.PccxError(f"train_ipdae: batch must be (B, {self.N}, 3), got {tuple(batch_x.shape)}")
        lam = 0.0 if self.global_step < self.rate_loss_enable_step else self.lamda    # :218-221
        if self.deterministic:
            # Adam's bias corrections from the DEVICE state, as the captured step has them (make_capturable): the host's powf and the
            # device's running double product differ in the last bit, and the eager and the replayed step are to give the same bits
            self.opt.make_capturable(batch_x.device)
        with train.step_scope(batch_x.device, None, self.autocast, self.opt.params, deterministic=self.deterministic) as forward_done:     # :173 optimizer.zero_grad()
            loss, fbpp, bpp = forward_loss(self.ae, self.prob, batch_x, starts, lam, self.S, self.K, self.N, self.N0, self.octree_mode)
            forward_done()
            loss.backward()                                                           # :229
            self.opt.step(max_norm=None)                                              # :230
        self.global_step += 1                                                         # :236
        if self.global_step % self.lr_decay_steps == 0:                               # :250-254
            self.lr *= self.lr_decay
            self.opt.set_lr(self.lr)
        return dict(loss=float(loss.detach()), fbpp=float(fbpp.detach()), bpp=float(bpp.detach()))

    def ragged_refusal(self, n_points, B, N_cap, S_cap=None):
        """Why step_ragged / RaggedGraphedIpdaeStep cannot take B clouds of these point counts in a slab of N_cap rows and S_cap
        patches per cloud: a message naming the limit and the way out, or None.  Host only, before any launch.  The shape rule is the
        codec's own (codec.ragged_shape_refusal)."""
        from . import codec
        if self.octree_mode != "full":
            return (f"ragged training needs octree_mode='full' (octree_mode='reference' is S = 64 by definition), got "
                    f"{self.octree_mode!r}: build the trainer with octree_mode='full' (train.py --octree-mode full)")
        if self.deterministic:
            return ("ragged training has no deterministic form (the ordered scatter of pccx_chamfer_grad_det is dense only): build the "
                    "trainer with deterministic=False, or train on one size per step")
        n = [int(v) for v in n_points]
        if len(n) != B:
            return f"{len(n)} point counts for {B} clouds: one count per cloud is expected"
        why = codec.ragged_shape_refusal(n, self.K, self.ALPHA, N_cap)
        if why is None and S_cap is not None and max(v * self.ALPHA // self.K for v in n) > S_cap:
            why = (f"a cloud of {max(n)} points has {max(n) * self.ALPHA // self.K} patches, the step holds S_cap = {S_cap} per cloud: "
                   f"build it with a larger S_cap, or send such clouds through step_ragged")
        return why

    def _ragged_tables(self, n_points):
        """(n, S, scale, plan) of a ragged batch: host tensors (int32, int32, float32) and the codec.ragged_plan they come from"""
        from . import codec
        plan = codec.ragged_plan(n_points, self.K, self.ALPHA, self.N0, self.ae.d)
        return (torch.tensor([int(v) for v in n_points], dtype=torch.int32), torch.tensor(plan.S, dtype=torch.int32),
                torch.tensor(plan.scale_compress, dtype=torch.float32), plan)

    def step_ragged(self, pc, n_points, starts, S_cap=None):
        """step for clouds of different sizes: pc (B, N_cap, 3) on the device with cloud b in its first n_points[b] rows (codec.pad_clouds),
        n_points a host sequence, starts the FPS start index per cloud in [0, n_b).  S_cap: the patches every cloud is padded to
        (default 16 * ceil(max S_b / 16), codec.ragged_plan's S_pad); a cloud's figures do not depend on it, nor on N_cap or the
        batch.  The loss is forward_loss_ragged's.  Same bookkeeping as step.  Refused with PccxError before any launch: what
        ragged_refusal names."""
        if pc.dim() != 3 or pc.shape[2] != 3:
            raise _lib.PccxError(f"train_ipdae: a ragged batch must be (B, N_cap, 3), got {tuple(pc.shape)}")
        B, N_cap = int(pc.shape[0]), int(pc.shape[1])
        why = self.ragged_refusal(n_points, B, N_cap, S_cap)
        if why:
            raise _lib.PccxError("train_ipdae: step_ragged: " + why)
        n, S, scale, plan = self._ragged_tables(n_points)
        S_cap = plan.S_pad if S_cap is None else int(S_cap)
        dev = pc.device
        n, S, scale = n.to(dev), S.to(dev), scale.to(dev)
        starts = ops.counts(starts, B, dev, "step_ragged.starts")
        lam = 0.0 if self.global_step < self.rate_loss_enable_step else self.lamda    # :218-221
        with train.step_scope(dev, None, self.autocast, self.opt.params) as forward_done:
            loss, fbpp, bpp = forward_loss_ragged(self.ae, self.prob, pc, n, S, scale, starts, lam, S_cap, self.K)
            forward_done()
            loss.backward()                                                           # :229
            self.opt.step(max_norm=None)                                              # :230
        self.global_step += 1                                                         # :236
        if self.global_step % self.lr_decay_steps == 0:                               # :250-254
            self.lr *= self.lr_decay
            self.opt.set_lr(self.lr)
        return dict(loss=float(loss.detach()), fbpp=float(fbpp.detach()), bpp=float(bpp.detach()))

    def graphed_ragged(self, N_cap, S_cap, B, pc, n_points, starts, warmup=2, keep_graph=False):
        """-> RaggedGraphedIpdaeStep at the capacities (N_cap points, S_cap patches, B clouds); the warm-up iterations are real steps
        on (pc, n_points, starts)"""
        return RaggedGraphedIpdaeStep(self, N_cap, S_cap, B, pc, n_points, starts, warmup, keep_graph)

    def validate_ragged(self, clouds, starts, **codec_kw):
        """validate for clouds of different sizes: clouds a list of (n_b, 3) device tensors, starts the FPS start index per cloud ->
        dict(bpp = the mean true rate of compress_ragged's three files, d1_psnr = the mean over the clouds of codec.d1_psnr on the
        unpadded pair (cloud, its decompress_ragged), n = B).  Repacks first, as validate explains."""
        from . import codec
        comp, outs = self.validation_pass_ragged(clouds, starts, **codec_kw)
        psnr = [float(codec.d1_psnr(c[None].to(torch.float32).contiguous(), o[None].contiguous())[0]) for c, o in zip(clouds, outs)]
        return dict(bpp=float(comp.bpp().mean()), d1_psnr=sum(psnr) / len(psnr), n=len(clouds))

    def validation_pass_ragged(self, clouds, starts, **codec_kw):
        """validate_ragged's codec run itself -> (the Compressed, the list of decompressed clouds (S_b*k, 3)); repacks first"""
        from . import codec
        pc, n = codec.pad_clouds(clouds)
        with torch.no_grad():
            self.ae.pack(pc.device)
            self.prob.pack(pc.device)
            cd = codec.Codec(self.ae, self.prob, self.K, self.ALPHA, self.N0, octree_mode=self.octree_mode, **codec_kw)
            comp = cd.compress_ragged(pc, n, starts)
            return comp, cd.decompress_ragged(comp, [v * self.ALPHA // self.K for v in n])

    def validate(self, clouds, starts, **codec_kw):
        """The current weights through the real codec: clouds (B, N, 3) on the device, starts the FPS start index per cloud ->
        dict(bpp = the mean true rate, Compressed.bpp(): the bits of the three files, not the estimate of the loss; d1_psnr = the mean
        codec.d1_psnr of decompress(compress(clouds)); n = B).  The codec is codec.Codec(ae, prob, K, ALPHA, N0, octree_mode of this
        trainer, **codec_kw), run under torch.no_grad().

        ae.pack() and prob.pack() come FIRST, and must: the codec reads the weights from packed blobs (AE._enc_blob / _dec_blob /
        _derived_blobs, the probability model's _blob, the generic layers' packed copies) that only pack() and load_state_dict() drop,
        while Adam moves the parameters in place -- without the two calls a codec built after a training step would still code with the
        weights of the last pack.  Training itself never reads a blob, so nothing else needs the calls."""
        from . import codec
        comp, out = self.validation_pass(clouds, starts, **codec_kw)
        return dict(bpp=float(comp.bpp().mean()), d1_psnr=float(codec.d1_psnr(clouds, out).mean()), n=int(clouds.shape[0]))

    def validation_pass(self, clouds, starts, **codec_kw):
        """validate's codec run itself -> (the Compressed, the decompressed clouds (B, S*k, 3)); repacks first, as validate explains"""
        from . import codec
        if clouds.dim() != 3 or clouds.shape[1] != self.N or clouds.shape[2] != 3:
            raise _lib.PccxError(f"train_ipdae: validate takes (B, {self.N}, 3), got {tuple(clouds.shape)}")
        with torch.no_grad():
            self.ae.pack(clouds.device)
            self.prob.pack(clouds.device)
            cd = codec.Codec(self.ae, self.prob, self.K, self.ALPHA, self.N0, octree_mode=self.octree_mode, **codec_kw)
            comp = cd.compress(clouds, starts)
            return comp, cd.decompress(comp, S=self.S)

    def graphed(self, batch_x, starts, warmup=2, keep_graph=False):
        """-> GraphedIpdaeStep over this trainer's models and optimizer (the warm-up iterations are real steps on batch_x)"""
        return GraphedIpdaeStep(self, batch_x, starts, warmup, keep_graph)


class GraphedIpdaeStep:
    """IpdaeTrainer.step captured ONCE as a hipGraph and replayed: the iteration is ~400 small launches at the reference's batch size of 1
    (64 patches), bound by launch latency, not by arithmetic.  Selection included: FPS, the octree depth search / encode / decode and
    both kNN searches are stream-ordered kernels that read the batch and the start indices from device memory.  What changes from step to
    step lives in buffers the graph reads: the batch, the start indices, lambda (0 until rate_loss_enable_step) and Adam's lr / bias
    corrections (Adam.make_capturable).  Shapes are fixed at construction."""

    def __init__(self, trainer, batch_x, starts, warmup=2, keep_graph=False):
        tr = self.tr = trainer
        dev = batch_x.device
        self.arena = train.StepArena()
        tr.opt.make_capturable(dev)
        self.x = batch_x.detach().to(torch.float32).clone().contiguous()
        self.starts = torch.as_tensor(starts).to(device=dev, dtype=torch.int32).contiguous().clone()
        self.lam = torch.zeros((), device=dev, dtype=torch.float32)
        self.warm_out = None

        def warm():
            self._set_lam()
            self.warm_out = self._body()                             # (loss, fbpp, bpp) of the last warm-up iteration, device scalars
            self._advance()
        self.graph, self.out, self._grads, _, _ = train.capture_step(dev, tr.opt, warmup, warm, self._body, keep_graph=keep_graph)

    def _set_lam(self):
        self.lam.fill_(0.0 if self.tr.global_step < self.tr.rate_loss_enable_step else self.tr.lamda)

    def _advance(self):
        tr = self.tr
        tr.global_step += 1
        if tr.global_step % tr.lr_decay_steps == 0:
            tr.lr *= tr.lr_decay
            tr.opt.set_lr(tr.lr)

    def _body(self):
        tr = self.tr
        with train.step_scope(self.x.device, self.arena, tr.autocast, tr.opt.params, deterministic=tr.deterministic) as forward_done:
            loss, fbpp, bpp = forward_loss(tr.ae, tr.prob, self.x, self.starts, self.lam, tr.S, tr.K, tr.N, tr.N0, tr.octree_mode)
            forward_done()
            loss.backward()
            tr.opt.step(max_norm=None)
        return loss.detach(), fbpp.detach(), bpp.detach()

    def __call__(self, batch_x=None, starts=None, sync=True):
        """one iteration on (batch_x, starts) (None = the buffers' current content) -> dict of floats, or of device scalars (sync=False)"""
        if batch_x is not None:
            self.x.copy_(batch_x)
        if starts is not None:
            self.starts.copy_(torch.as_tensor(starts).to(self.x.device, torch.int32))
        self._set_lam()
        self.graph.replay()
        self.tr.opt.t += 1
        self._advance()
        keys = ("loss", "fbpp", "bpp")
        return {k: float(v) for k, v in zip(keys, self.out)} if sync else dict(zip(keys, self.out))


class RaggedGraphedIpdaeStep:
    """IpdaeTrainer.step_ragged captured ONCE at capacities (B clouds of up to N_cap points and S_cap patches) and replayed on any batch
    with n_b <= N_cap and S_b <= S_cap.  The batch, the per-cloud tables n / S / scale, the start indices, lambda and Adam's scalars
    live in buffers the graph reads; shapes, grids and S_cap are fixed at construction, so every replay does the matrix work of
    B * S_cap patches whatever the clouds hold.  Built on train.capture_step / step_scope as GraphedIpdaeStep is."""

    def __init__(self, trainer, N_cap, S_cap, B, pc, n_points, starts, warmup=2, keep_graph=False):
        tr = self.tr = trainer
        self.N_cap, self.S_cap, self.B = int(N_cap), int(S_cap), int(B)
        why = tr.ragged_refusal(n_points, self.B, self.N_cap, self.S_cap)
        if why:
            raise _lib.PccxError("train_ipdae: graphed_ragged: " + why)
        dev = pc.device
        self.arena = train.StepArena()
        tr.opt.make_capturable(dev)
        self.x = torch.zeros(self.B, self.N_cap, 3, device=dev, dtype=torch.float32)
        self.n = torch.zeros(self.B, device=dev, dtype=torch.int32)
        self.S = torch.zeros(self.B, device=dev, dtype=torch.int32)
        self.scale = torch.ones(self.B, device=dev, dtype=torch.float32)
        self.starts = torch.zeros(self.B, device=dev, dtype=torch.int32)
        self.lam = torch.zeros((), device=dev, dtype=torch.float32)
        self.warm_out = None
        self._load(pc, n_points, starts)

        def warm():
            self._set_lam()
            self.warm_out = self._body()                             # (loss, fbpp, bpp) of the last warm-up iteration, device scalars
            self._advance()
        self.graph, self.out, self._grads, _, _ = train.capture_step(dev, tr.opt, warmup, warm, self._body, keep_graph=keep_graph)

    def _load(self, pc, n_points, starts):
        """a batch into the buffers the graph reads; refused on the host, before any copy, as step_ragged refuses"""
        tr = self.tr
        if pc.dim() != 3 or pc.shape[0] != self.B or pc.shape[1] > self.N_cap or pc.shape[2] != 3:
            raise _lib.PccxError(f"train_ipdae: this captured step takes ({self.B}, <= {self.N_cap}, 3), got {tuple(pc.shape)}")
        why = tr.ragged_refusal(n_points, self.B, int(pc.shape[1]), self.S_cap)
        if why:
            raise _lib.PccxError("train_ipdae: graphed_ragged: " + why)
        n, S, scale, _ = tr._ragged_tables(n_points)
        self.x[:, :pc.shape[1]].copy_(pc)
        self.n.copy_(n)
        self.S.copy_(S)
        self.scale.copy_(scale)
        self.starts.copy_(torch.as_tensor(starts).to(self.x.device, torch.int32))

    _set_lam = GraphedIpdaeStep._set_lam
    _advance = GraphedIpdaeStep._advance

    def _body(self):
        tr = self.tr
        with train.step_scope(self.x.device, self.arena, tr.autocast, tr.opt.params) as forward_done:
            loss, fbpp, bpp = forward_loss_ragged(tr.ae, tr.prob, self.x, self.n, self.S, self.scale, self.starts, self.lam, self.S_cap, tr.K)
            forward_done()
            loss.backward()
            tr.opt.step(max_norm=None)
        return loss.detach(), fbpp.detach(), bpp.detach()

    def __call__(self, pc=None, n_points=None, starts=None, sync=True):
        """one iteration on (pc, n_points, starts) (None = the buffers' current content) -> dict of floats, or of device scalars
        (sync=False)"""
        if pc is not None:
            self._load(pc, n_points, starts)
        self._set_lam()
        self.graph.replay()
        self.tr.opt.t += 1
        self._advance()
        keys = ("loss", "fbpp", "bpp")
        return {k: float(v) for k, v in zip(keys, self.out)} if sync else dict(zip(keys, self.out))


def crop_locate(sizes, draws):
    """(cloud, index inside it) of global point indices into a store whose clouds hold ``sizes`` points, in store order (host only):
    a draw uniform over all points of the store lands in a cloud in proportion to its size."""
    import bisect
    ends, total = [], 0
    for s in sizes:
        total += int(s)
        ends.append(total)
    out = []
    for g in (int(v) for v in draws):
        if not 0 <= g < total:
            raise _lib.PccxError(f"crop_locate: point {g} is outside a store of {total} points")
        c = bisect.bisect_right(ends, g)
        out.append((c, g - (ends[c] - int(sizes[c]))))
    return [c for c, _ in out], [i for _, i in out]


class CropSampler:
    """Training crops of a store of clouds of any size (codec.pack_clouds): every draw cuts B compact crops, each the n points nearest
    to a seed point (ops.crop_nearest: exact, ties to the lower index, the file's own order), on the current stream into ONE buffer
    this sampler owns, (B, N_cap, 3) with NaN behind each crop -- the batch IpdaeTrainer.step (n = N_cap) and step_ragged /
    RaggedGraphedIpdaeStep take as it is.  The seed points are drawn on the host from ``generator`` (a CPU torch.Generator), uniformly
    over ALL points of the store, so a room contributes in proportion to its size; two samplers seeded alike draw the same crops."""

    def __init__(self, points, offsets, sizes, B, N_cap, generator):
        self.sizes = [int(v) for v in sizes]
        self.B, self.N_cap = int(B), int(N_cap)
        if not isinstance(generator, torch.Generator) or generator.device.type != "cpu":
            raise _lib.PccxError("CropSampler: generator must be a CPU torch.Generator (the seed points are drawn on the host)")
        if not 1 <= self.B <= ops.CROP_MAX_B:
            raise _lib.PccxError(f"CropSampler: B={self.B}; one draw cuts 1..CROP_MAX_B = {ops.CROP_MAX_B} crops")
        if not 1 <= self.N_cap <= ops.CROP_MAX_NCAP:
            raise _lib.PccxError(f"CropSampler: N_cap={self.N_cap}; a crop holds 1..CROP_MAX_NCAP = {ops.CROP_MAX_NCAP} points")
        if not self.sizes or min(self.sizes) < 1 or max(self.sizes) > ops.CROP_MAX_M:
            raise _lib.PccxError(f"CropSampler: every cloud must hold 1..CROP_MAX_M = {ops.CROP_MAX_M} points, got "
                                 f"{min(self.sizes) if self.sizes else 'no cloud'}..{max(self.sizes) if self.sizes else ''}")
        if (not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32
                or points.shape[0] != sum(self.sizes)):
            raise _lib.PccxError(f"CropSampler: points must be ({sum(self.sizes)}, 3) float32 for clouds of these sizes (codec.pack_clouds), got "
                                 f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
        if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or tuple(offsets.shape) != (len(self.sizes) + 1,):
            raise _lib.PccxError(f"CropSampler: offsets must be ({len(self.sizes) + 1},) int64 (codec.pack_clouds)")
        self.points, self.offsets, self.generator = ops._f32c(points, "CropSampler.points"), offsets, generator
        self.M_total = int(points.shape[0])
        dev = points.device
        self.batch = torch.empty(self.B, self.N_cap, 3, device=dev, dtype=torch.float32)
        self.idx = torch.empty(self.B, self.N_cap, device=dev, dtype=torch.int32)
        self.workspace = torch.empty(int(_lib.load().pccx_crop_nearest_workspace_bytes(self.B, max(self.sizes))), device=dev, dtype=torch.uint8)

    def _counts(self, n):
        n = [int(n)] * self.B if isinstance(n, int) else [int(v) for v in n]
        if len(n) != self.B:
            raise _lib.PccxError(f"CropSampler: {len(n)} counts for {self.B} crops: one int, or one per crop, is expected")
        return n

    def _starts(self, n):
        # the draw of pn_kit.py:321 inside each crop, as cli/train.py draws it for a ragged batch
        return torch.cat([torch.randint(0, nb, (1,), dtype=torch.long, generator=self.generator) for nb in n])

    def draw_fixed(self, cloud_ids, seeds, n):
        """the crops of caller-chosen seed points: cloud_ids / seeds host lists of B ints, n one int or B -> (batch, n list, starts);
        everything is range-checked on the host before the launch (ops.crop_nearest), nothing is capped"""
        n = self._counts(n)
        ops.crop_nearest(self.points, self.offsets, [int(c) for c in cloud_ids], [int(s) for s in seeds], n, self.N_cap,
                         workspace=self.workspace, sizes=self.sizes, out=self.batch, out_idx=self.idx)
        return self.batch, n, self._starts(n)

    def draw(self, n):
        """B crops of n points (one int, or a list of B) around seed points drawn uniformly over all points of the store: ONE
        torch.randint over M_total, mapped to (cloud, index) by crop_locate; a count above its cloud's size is capped at it.
        -> (batch (B, N_cap, 3): the sampler's own buffer, overwritten by the next draw; n list; starts: the FPS start index of
        each crop, (B,) int64 on the host)"""
        n = self._counts(n)
        g = torch.randint(0, self.M_total, (self.B,), dtype=torch.long, generator=self.generator)
        cloud_ids, seeds = crop_locate(self.sizes, g.tolist())
        return self.draw_fixed(cloud_ids, seeds, [min(v, self.sizes[c]) for v, c in zip(n, cloud_ids)])
