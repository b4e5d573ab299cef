"""GPU parity: the neural transforms (fp32 MFMA chains) vs golden fixtures and the torch oracle.

Tolerances (floating point, stated per assert): the HIP path accumulates each dot product as a
k-ordered fp32 fmaf chain on the matrix cores, torch CPU uses oneDNN/MKL blocked sums, so results
agree to ~1e-6 relative, not bit-for-bit.  Quantised symbols must be identical except where the
pre-rounding value sits within 1e-4 of a rounding boundary.
"""
import os

import numpy as np
import pytest
import torch

from oracle import cport, ref_model
from pccx import models, ops
from tests import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
K, k, d, L = synth.MODEL_CFG


@pytest.fixture(autouse=True, params=["f32", "bf16x3", "f16x2"])
def matmul_mode(request):
    """Every test of this module runs in ALL arithmetic modes of the three transforms at the SAME tolerances against
    the oracle / golden fixtures: exact-fp32 MFMA, fp32 products formed from three bf16 pieces per operand, and fp32 products
    formed from two scaled fp16 pieces per operand (the fused encoder / decoder; other kernels run bf16x3 in that mode)."""
    import pccx
    old = pccx.DEFAULT_MATMUL
    pccx.DEFAULT_MATMUL = request.param
    yield request.param
    pccx.DEFAULT_MATMUL = old


@pytest.fixture(scope="module")
def nets():
    ae = models.AE(K, k, d, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    prob = models.ConditionalProbabilityModel(L, d)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    oae = ref_model.AE(K, k, d, L).eval()
    oae.load_state_dict(ae.state_dict())
    oprob = ref_model.ConditionalProbabilityModel(L, d).eval()
    oprob.load_state_dict(prob.state_dict())
    return ae.pack("cuda"), prob.pack("cuda"), oae, oprob


def _symbols_agree(q_gpu, latent_ref, q_ref):
    bad = q_gpu != q_ref
    if bad.any():
        frac = np.abs(latent_ref[bad] - np.floor(latent_ref[bad]) - 0.5)
        assert (frac < 1e-4).all(), f"{bad.sum()} symbol flips away from a rounding boundary"
    return int(bad.sum())


def test_state_dict_keys_match_reference(nets):
    md = np.load(os.path.join(G, "model.npz"))
    ae, prob = nets[0], nets[1]
    assert list(ae.state_dict().keys()) == list(md["ae_keys"])
    assert [str(tuple(v.shape)) for v in ae.state_dict().values()] == list(md["ae_shapes"])
    assert list(prob.state_dict().keys()) == list(md["prob_keys"])


def test_encoder_matches_golden(nets):
    md = np.load(os.path.join(G, "model.npz"))
    ae = nets[0]
    patches = torch.from_numpy(synth.patch_batch(K)).cuda()
    raw, latent, q = ae.encode(patches)
    np.testing.assert_allclose(raw.cpu().numpy(), md["pn_latent_raw"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(latent.cpu().numpy(), md["ae_latent"], rtol=0, atol=5e-5)
    _symbols_agree(q.cpu().numpy(), md["ae_latent"], md["ae_latent_q"])


def test_decoder_matches_golden(nets):
    md = np.load(os.path.join(G, "model.npz"))
    ae = nets[0]
    lq = torch.from_numpy(synth.latent_case(2, d, L)).cuda()
    out = ae.decode(lq)
    np.testing.assert_allclose(out.cpu().numpy(), md["dec_out"], rtol=1e-4, atol=2e-5)
    rec, latent, q = ae(torch.from_numpy(synth.patch_batch(K)).cuda())
    same = (q.cpu().numpy() == md["ae_latent_q"]).all(axis=1)                  # patches whose 16 symbols all equal the reference's
    assert same.mean() >= 0.9, "too few patches reproduce the reference's symbols for the reconstruction fixture to apply"
    np.testing.assert_allclose(rec.cpu().numpy()[same], md["ae_recon"][same], rtol=1e-4, atol=2e-5)
    with torch.no_grad():                                                       # every patch, against the oracle fed the GPU's symbols
        want = nets[2].decode(q.cpu())
    np.testing.assert_allclose(rec.cpu().numpy(), want.numpy(), rtol=1e-4, atol=2e-5)


def test_prob_model_matches_golden(nets):
    md = np.load(os.path.join(G, "model.npz"))
    prob = nets[1]
    r = prob.run(torch.from_numpy(synth.centres_case()).cuda(), ("pmf", "cdf", "cdf_int"))
    np.testing.assert_allclose(r["pmf"].cpu().numpy(), md["pmf"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(r["cdf"].cpu().numpy(), md["cdf"], rtol=0, atol=4e-6)
    want = ref_model.cdf_float_to_int(torch.from_numpy(md["cdf"]))
    got = r["cdf_int"].cpu().numpy()
    diff = ((got.astype(np.int64) - want.astype(np.int64) + 32768) % 65536) - 32768
    assert np.abs(diff).max() <= 1          # +-1 count where the float cdf differs in its last bits


@pytest.mark.parametrize("P", [1, 5, 37])
def test_encoder_decoder_vs_oracle_ragged_batches(nets, P):
    ae, _, oae, _ = nets
    rng = np.random.default_rng(P)
    base = synth.patch_batch(K, P=min(P, 6), seed=70 + P)
    patches = np.concatenate([base] * ((P + base.shape[0] - 1) // base.shape[0]))[:P].copy()
    patches += rng.normal(0, 1e-3, patches.shape).astype(np.float32)
    x = torch.from_numpy(patches)
    torch.set_num_threads(8)
    with torch.no_grad():
        olat = oae.encode(x)
        oq = olat.round()
        odec = oae.decode(oq)
    raw, latent, q = ae.encode(x.cuda())
    np.testing.assert_allclose(latent.cpu().numpy(), olat.numpy(), rtol=0, atol=5e-5)
    flips = _symbols_agree(q.cpu().numpy(), olat.numpy(), oq.numpy())
    dec = ae.decode(oq.cuda())
    np.testing.assert_allclose(dec.cpu().numpy(), odec.numpy(), rtol=1e-4, atol=2e-5)
    assert flips <= max(1, P * d // 200)


def test_sa_knn_ties_on_lattice_patch(nets):
    """Lattice patch: many equal in-patch distances; the kNN-16 tie rule (lower index) must match."""
    ae, _, oae, _ = nets
    rng = np.random.default_rng(0)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    patches = ((g[rng.permutation(256)] - 3.5) * 0.05).astype(np.float32)[None]
    with torch.no_grad():
        olat = oae.encode(torch.from_numpy(patches))
    _, latent, _ = ae.encode(torch.from_numpy(patches).cuda())
    np.testing.assert_allclose(latent.cpu().numpy(), olat.numpy(), rtol=0, atol=5e-5)


def _sa_features(ae, patches):
    """ae.sa as the reference calls it (compress.py:113-115): [P,3,K] -> (new_xyz, features [P,128,K]), current matmul mode."""
    x = torch.from_numpy(patches).cuda().permute(0, 2, 1)
    new_xyz, feat = ae.sa(x)
    assert torch.equal(new_xyz, x)                      # npoint == K: the points themselves (pn_kit.py:180-181)
    return feat.cpu().numpy()


def test_sa_feature_map_with_ties_and_near_ties_at_the_16th_neighbour(nets):
    """The in-patch kNN-16 selects with the candidate index packed into the low bits of the distance and
    falls back to the exact (distance, index) rule when ranks 16 and 17 agree in the kept bits.  Patches
    built to hit both sides of that test: exact ties (lattice), distances that differ only in the last few
    mantissa bits (a jittered shell around point 0, seen from point 0 every neighbour is a near-tie),
    duplicated points, and an ordinary random patch.  A wrong neighbour changes that point's features far
    beyond the tolerance."""
    ae, _, oae, _ = nets
    rng = np.random.default_rng(5)
    lattice = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    lattice = ((lattice[rng.permutation(256)] - 3.5) * 0.05).astype(np.float32)
    dirs = rng.normal(size=(255, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    radius = 0.3 * (1.0 + rng.integers(-40, 41, size=(255, 1)) * 2.0 ** -24)      # +-40 ulp of radial jitter
    shell = np.concatenate([np.zeros((1, 3)), dirs * radius]).astype(np.float32)
    dup = rng.uniform(-0.4, 0.4, size=(128, 3)).astype(np.float32)
    dup = np.concatenate([dup, dup])[rng.permutation(256)]
    rand = rng.uniform(-0.5, 0.5, size=(256, 3)).astype(np.float32)
    patches = np.stack([lattice, shell, dup, rand])
    got = _sa_features(ae, patches)
    with torch.no_grad():
        _, want = oae.sa(torch.from_numpy(patches).permute(0, 2, 1))
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-4, atol=1e-4)


def test_decode_reassembly_matches_decompress_ops(nets):
    """pc_out path = decompress.py:104-116: / scale, + centres, denormalize."""
    ae, _, oae, _ = nets
    S, B = 64, 2
    rng = np.random.default_rng(4)
    lq = rng.integers(-3, 4, size=(B * S, d)).astype(np.float32)
    centres = ((rng.integers(0, 128, size=(B, S, 3)) + 0.5) / 128).astype(np.float32)
    center = rng.normal(size=(B, 3)).astype(np.float32)
    longest = (1 + rng.random(B)).astype(np.float32)
    scale = float((S * k / 1024) ** (1 / 3))
    pc = ae.decode(torch.from_numpy(lq).cuda(), torch.from_numpy(centres).cuda(), torch.from_numpy(center).cuda(),
                   torch.from_numpy(longest).cuda(), S=S, scale=scale)
    raw = ae.decode(torch.from_numpy(lq).cuda()).cpu()
    patches = raw / scale
    want = (patches.view(B, S, -1, 3) + torch.from_numpy(centres).view(B, S, 1, 3)).reshape(B, -1, 3)
    for b in range(B):
        w = ref_model.denormalize(want[b:b + 1], torch.from_numpy(center[b]).reshape(1, 3), torch.from_numpy(longest[b:b + 1]))
        assert np.array_equal(pc[b].cpu().numpy(), w[0].numpy())      # same fp32 op sequence: bit-exact


def test_range_coder_device_matches_oracle_bytes_and_round_trips(nets):
    prob = nets[1]
    rng = np.random.default_rng(6)
    B, S = 9, 64
    centres = ((rng.integers(0, 128, size=(B, S, 3)) + 0.5) / 128).astype(np.float32)
    r = prob.run(torch.from_numpy(centres).cuda(), ("pmf", "cdf_int"))
    pmf = r["pmf"].cpu().numpy().reshape(B, S * d, L).astype(np.float64)
    sym = np.stack([[rng.choice(L, p=row / row.sum()) for row in pmf[b]] for b in range(B)])
    sym[0] = 0; sym[1] = L - 1                                   # degenerate streams
    q = (sym - L // 2).astype(np.float32)
    by, nb = models.range_encode(r["cdf_int"], torch.from_numpy(q).cuda(), L)
    back = models.range_decode(r["cdf_int"], by, nb, L)
    assert np.array_equal(back.cpu().numpy(), q)                 # lossless on device
    ci = r["cdf_int"].cpu().numpy().reshape(B, S * d, L + 1)
    tot_ideal = 0.0
    for b in range(B):
        want = cport.range_encode(ci[b], sym[b].astype(np.int16))
        got = bytes(by[b, :int(nb[b])].cpu().numpy())
        assert got == want                                       # byte-identical to the oracle coder
        assert np.array_equal(cport.range_decode(ci[b], got), sym[b])
        tot_ideal += -np.log2(pmf[b][np.arange(S * d), sym[b]]).sum() / 8
    assert abs(int(nb.sum()) - tot_ideal) <= 0.01 * tot_ideal + 2 * B


def test_range_coder_adversarial_tables_match_oracle_bit_for_bit():
    """Hand-made CDF tables that force long E3 (underflow) runs, long E1/E2 runs and 1-count
    symbols: the bulk-renormalising device coder must equal the oracle's literal one-bit-at-a-time
    restatement byte for byte, and decode back losslessly."""
    rng = np.random.default_rng(12)
    B, nsym, Lp = 24, 1024, 8
    cdf = np.zeros((B, nsym, Lp), dtype=np.int64)
    sym = np.zeros((B, nsym), dtype=np.int64)
    for b in range(B):
        kind = b % 6
        for i in range(nsym):
            if kind == 0:      # a sliver around the midpoint: symbol 3 straddles 0x8000 -> E3 runs
                t = [0, 1, 2, 0x7FFF, 0x8001, 0xFFFD, 0xFFFE]
                s = 3
            elif kind == 1:    # 1-count symbols everywhere
                t = [0] + sorted(rng.choice(np.arange(1, 0xFFFF), size=6, replace=False).tolist())
                s = int(rng.integers(0, 7))
            elif kind == 2:    # near-certain symbol, occasional rare ones
                t = [0, 1, 2, 3, 4, 5, 0xFFFF]
                s = 5 if rng.random() < 0.97 else int(rng.integers(0, 7))
            elif kind == 3:    # alternate the two slivers either side of 0x8000
                t = [0, 0x2000, 0x4000, 0x7FFF, 0x8000, 0x8001, 0xC000]
                s = 3 + (i & 1)
            elif kind == 4:    # uniform
                t = [int(j * 65536 / 7) for j in range(7)]
                s = int(rng.integers(0, 7))
            else:              # random monotone table, random symbols
                t = [0] + sorted(rng.choice(np.arange(1, 0xFFFF), size=6, replace=False).tolist())
                s = int(rng.integers(0, 7))
            cdf[b, i, :7] = t
            cdf[b, i, 7] = 0          # entry Lp-1 is 0x10000 wrapped to 16 bits, as torchac stores it
            sym[b, i] = s
    q = (sym - 3).astype(np.float32)
    ci = torch.from_numpy(cdf.astype(np.int32)).cuda()
    by, nb = models.range_encode(ci, torch.from_numpy(q).cuda(), 7, cap=8192)
    assert (nb > 0).all()
    back = models.range_decode(ci, by, nb, 7)
    assert np.array_equal(back.cpu().numpy(), q)
    for b in range(B):
        want = cport.range_encode(cdf[b].astype(np.int32), sym[b].astype(np.int16))
        assert bytes(by[b, :int(nb[b])].cpu().numpy()) == want, f"stream {b} (kind {b % 6})"
        assert np.array_equal(cport.range_decode(cdf[b].astype(np.int32), want), sym[b])


@pytest.mark.parametrize("L,nsym", [(3, 1000), (2, 77), (15, 1024), (31, 130), (62, 257), (63, 64), (64, 200), (7, 1)])
def test_range_coder_other_alphabets_and_ragged_lengths(L, nsym):
    """Alphabet sizes that change the lane layout of the device decoder (64 // (L+1) symbols per block of
    lanes; L = 64 takes the one-lane-per-cloud kernel) and stream lengths that are not multiples of a
    block: bytes equal the oracle's, and the round trip is lossless."""
    rng = np.random.default_rng(100 * L + nsym)
    B, Lp = 5, L + 1
    cdf = np.zeros((B, nsym, Lp), dtype=np.int64)
    sym = rng.integers(0, L, size=(B, nsym))
    for b in range(B):
        for i in range(nsym):
            if b == 0:        # uniform-ish
                cdf[b, i, :L] = (np.arange(L) * 65536) // L
            elif b == 1:      # one dominant symbol, 1-count rest
                k = int(rng.integers(0, L))
                w = np.ones(L, dtype=np.int64); w[k] = 65536 - (L - 1)
                cdf[b, i, 1:L] = np.cumsum(w)[:-1]
            else:             # random strictly increasing
                cdf[b, i, 1:L] = np.sort(rng.choice(np.arange(1, 0xFFFF), size=L - 1, replace=False))
    ci = torch.from_numpy(cdf.astype(np.int32)).cuda()
    q = (sym - L // 2).astype(np.float32)
    by, nb = models.range_encode(ci, torch.from_numpy(q).cuda(), L, cap=4 * nsym + 16)
    assert (nb > 0).all()
    back = models.range_decode(ci, by, nb, L)
    assert np.array_equal(back.cpu().numpy(), q)
    for b in range(B):
        want = cport.range_encode(cdf[b].astype(np.int32), sym[b].astype(np.int16))
        assert bytes(by[b, :int(nb[b])].cpu().numpy()) == want, f"stream {b}"
        assert np.array_equal(cport.range_decode(cdf[b].astype(np.int32), want), sym[b])


def test_decoder_bf16x3_matches_fp32_path(nets):
    """the decoder's 1024 -> k*128 Linear as fp32 products of three bf16 pieces per operand on
    the bf16 matrix cores.  Not bit-identical to the fp32 MFMA path; the bar is the same as any fp32 summation
    reorder: raw patches within 2e-6 absolute of the default path (values are O(0.1)) and within the decoder
    golden tolerance of the oracle."""
    ae, _, oae, _ = nets
    rng = np.random.default_rng(21)
    for P in (1, 37, 300):
        lq = rng.integers(-3, 4, size=(P, d)).astype(np.float32)
        a = ae.decode(torch.from_numpy(lq).cuda(), matmul="f32").cpu().numpy()
        b = ae.decode(torch.from_numpy(lq).cuda(), matmul="bf16x3").cpu().numpy()
        assert np.isfinite(b).all()
        assert np.abs(a - b).max() <= 2e-6 * max(1.0, np.abs(a).max()), (P, np.abs(a - b).max(), np.abs(a).max())
        with torch.no_grad():
            want = oae.decode(torch.from_numpy(lq)).numpy() if hasattr(oae, "decode") else None
        if want is not None:
            np.testing.assert_allclose(b, want.reshape(b.shape), rtol=1e-4, atol=2e-5)
    # the reassembled cloud path
    B, S = 2, 64
    lq = rng.integers(-3, 4, size=(B * S, d)).astype(np.float32)
    centres = rng.random((B, S, 3)).astype(np.float32)
    center = rng.random((B, 3)).astype(np.float32)
    longest = (rng.random(B) + 0.5).astype(np.float32)
    args = [torch.from_numpy(x).cuda() for x in (lq, centres, center, longest)]
    p0 = ae.decode(args[0], args[1], args[2], args[3], S=S, scale=2.0, matmul="f32").cpu().numpy()
    p1 = ae.decode(args[0], args[1], args[2], args[3], S=S, scale=2.0, matmul="bf16x3").cpu().numpy()
    assert np.abs(p0 - p1).max() <= 4e-6 * max(1.0, np.abs(p0).max())


def test_sa_bf16x3_matches_fp32_path(nets):
    """SetAbstraction conv1 / conv2 as bf16x3-split fp32 products.  Feature map within 1e-6 of the
    exact-fp32 kernel (features are O(0.1)), latents within 2e-6, symbols equal except at a rounding boundary."""
    from pccx import _lib
    ae = nets[0]
    patches = synth.patch_batch(K)
    x = torch.from_numpy(patches).cuda().contiguous()
    P = x.shape[0]
    enc, _ = ae._blobs(x.device)
    f0 = torch.empty(P * 8 * K * 16, device="cuda")
    f1 = torch.empty_like(f0)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("pccx_sa_forward", x.data_ptr(), P, K, enc.data_ptr(), f0.data_ptr(), st)
    _lib.call("pccx_sa_forward_b3", x.data_ptr(), P, K, enc.data_ptr(), ae._sa_b3_blob(x.device).data_ptr(), f1.data_ptr(), st)
    a, b = f0.cpu().numpy(), f1.cpu().numpy()
    assert np.abs(a - b).max() <= 1e-6 * max(1.0, np.abs(a).max()), (np.abs(a - b).max(), np.abs(a).max())
    _, lat0, q0 = ae.encode(x, sa_matmul="f32", pn_matmul="f32")
    _, lat1, q1 = ae.encode(x, sa_matmul="bf16x3", pn_matmul="f32")
    assert np.abs(lat0.cpu().numpy() - lat1.cpu().numpy()).max() <= 2e-6
    _symbols_agree(q1.cpu().numpy(), lat0.cpu().numpy(), q0.cpu().numpy())


def test_pointnet_bf16x3_matches_fp32_path(nets):
    """the PointNet chain (131->128->256->512->d) on bf16x3 operands, eight waves x one tile per pass,
    layer 2 k-outer in two halves.  Pre-sigmoid latents within 2e-5 relative of the exact-fp32 kernel (512-term sums of
    O(1) products), latents within 5e-6, symbols equal except at a rounding boundary; also against the oracle at the
    golden tolerance."""
    ae, _, oae, _ = nets
    patches = synth.patch_batch(K)
    x = torch.from_numpy(patches).cuda()
    raw0, lat0, q0 = ae.encode(x, sa_matmul="f32", pn_matmul="f32")
    raw1, lat1, q1 = ae.encode(x, sa_matmul="f32", pn_matmul="bf16x3")
    r0, r1 = raw0.cpu().numpy(), raw1.cpu().numpy()
    assert np.abs(r0 - r1).max() <= 2e-5 * max(1.0, np.abs(r0).max()), (np.abs(r0 - r1).max(), np.abs(r0).max())
    assert np.abs(lat0.cpu().numpy() - lat1.cpu().numpy()).max() <= 5e-6
    _symbols_agree(q1.cpu().numpy(), lat0.cpu().numpy(), q0.cpu().numpy())
    with torch.no_grad():
        olat = oae.encode(torch.from_numpy(patches))
    np.testing.assert_allclose(lat1.cpu().numpy(), olat.numpy(), rtol=0, atol=5e-5)
    # ragged: a patch count that leaves idle waves in the last pass is covered by K = 256 only (16 tiles = 2 passes);
    # all three experimental stages together
    raw2, lat2, q2 = ae.encode(x, sa_matmul="bf16x3", pn_matmul="bf16x3")
    assert np.abs(lat0.cpu().numpy() - lat2.cpu().numpy()).max() <= 5e-6


@pytest.mark.parametrize("Kx,kx,P", [(64, 32, 5), (512, 256, 3), (16, 8, 2)])
def test_bf16x3_other_patch_sizes(Kx, kx, P):
    """The bf16x3 kernels at other patch sizes (K = 16: one tile, seven of PointNet's eight waves idle;
    K = 512: four passes; other k for the decoder's per-point streams): same agreement with the exact-fp32 kernels."""
    ae = models.AE(Kx, kx, d, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    ae.pack("cuda")
    rng = np.random.default_rng(Kx + P)
    x = torch.from_numpy((rng.random((P, Kx, 3)).astype(np.float32) - 0.5)).cuda()
    raw0, lat0, q0 = ae.encode(x, sa_matmul="f32", pn_matmul="f32")
    raw1, lat1, q1 = ae.encode(x, sa_matmul="bf16x3", pn_matmul="bf16x3")
    assert np.abs(raw0.cpu().numpy() - raw1.cpu().numpy()).max() <= 2e-5 * max(1.0, float(raw0.abs().max()))
    assert np.abs(lat0.cpu().numpy() - lat1.cpu().numpy()).max() <= 5e-6
    _symbols_agree(q1.cpu().numpy(), lat0.cpu().numpy(), q0.cpu().numpy())
    a = ae.decode(q0, matmul="f32").cpu().numpy()
    b = ae.decode(q0, matmul="bf16x3").cpu().numpy()
    assert np.abs(a - b).max() <= 2e-6 * max(1.0, np.abs(a).max())


def _seeded_ae(Kx, kx, bias_gain=1.0):
    ae = models.AE(Kx, kx, d, L)
    sd = ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN)
    if bias_gain != 1.0:
        sd = {n: (v * bias_gain if n.endswith("bias") else v) for n, v in sd.items()}
    ae.load_state_dict(sd)
    return ae.pack("cuda")


def test_load_state_dict_leaves_no_stale_blob(matmul_mode):
    """New weights loaded into a packed AE that has already run: every blob made from the old ones (the packed fp32 pair and the five
    derived from it) is rebuilt, so the object computes bit for bit what a fresh AE with those weights does.  P = 5 is no multiple of
    the decoder's 16-patch tile, K = 32 the smallest K with two PointNet tiles."""
    Kx, kx, dx, P = 32, 16, 4, 5
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((P, Kx, 3)).astype(np.float32)).cuda()

    def run(ae):
        raw, lat, q = ae.encode(x, sa_matmul=matmul_mode, pn_matmul=matmul_mode)
        return raw, lat, q, ae.decode(q, matmul=matmul_mode)

    ae = models.AE(Kx, kx, dx, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    first = run(ae)
    sd2 = ref_model.seeded_state_dict(ae, synth.AE_SEED + 10, last_gain=synth.AE_LAST_GAIN)
    ae.load_state_dict(sd2)
    second = run(ae)
    fresh = models.AE(Kx, kx, dx, L)
    fresh.load_state_dict(sd2)
    for got, want in zip(second, run(fresh)):
        assert torch.equal(got, want)
    raw1, lat1, _, rec1 = first                           # (the 20 symbols alone could agree by chance)
    assert not torch.equal(second[0], raw1) and not torch.equal(second[1], lat1) and not torch.equal(second[3], rec1)


def test_prob_model_reload_drops_the_generic_layers():
    """The same guard for the probability model outside the fused kernel's shapes (d * L = 144 > 128): its generic layers, model_pn's
    and model_mlp's, are packed lazily on first use, and load_state_dict drops them."""
    Lx, dx = 9, 16
    x = torch.from_numpy(np.random.default_rng(4).random((2, 16, 3)).astype(np.float32)).cuda()
    prob = models.ConditionalProbabilityModel(Lx, dx)
    assert not prob.fused_ok(16)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    first = prob.run(x, ("pmf", "cdf_int"))
    sd2 = ref_model.seeded_state_dict(prob, synth.PROB_SEED + 10, gain=synth.PROB_GAIN)
    prob.load_state_dict(sd2)
    second = prob.run(x, ("pmf", "cdf_int"))
    fresh = models.ConditionalProbabilityModel(Lx, dx)
    fresh.load_state_dict(sd2)
    want = fresh.run(x, ("pmf", "cdf_int"))
    assert torch.equal(second["pmf"], want["pmf"]) and torch.equal(second["cdf_int"], want["cdf_int"])
    assert not torch.equal(second["pmf"], first["pmf"])


@pytest.mark.parametrize("Kx,kx,P", [(256, 128, 37), (64, 32, 5), (512, 256, 3), (16, 8, 2), (48, 24, 3)])
def test_f16x2_matches_fp32_path(Kx, kx, P):
    """The f16x2 kernels (csrc/encoder_fused_h2.hip, decoder_h2.hip: two scaled fp16 pieces per operand, three MFMA passes per
    fp32 product) against the exact-fp32 kernels at the bars of the bf16x3 tests above: pre-sigmoid latents within 2e-5 relative,
    latents within 5e-6, symbols equal except at a rounding boundary, decoder output within 2e-6; and against the oracle at the
    golden tolerances."""
    ae = _seeded_ae(Kx, kx)
    rng = np.random.default_rng(Kx * 7 + P)
    x = torch.from_numpy((rng.random((P, Kx, 3)).astype(np.float32) - 0.5)).cuda()
    x[0, : Kx // 2] = x[0, Kx // 2:]                                  # duplicated points
    raw0, lat0, q0 = ae.encode(x, sa_matmul="f32", pn_matmul="f32")
    raw1, lat1, q1 = ae.encode(x, sa_matmul="f16x2", pn_matmul="f16x2")
    assert torch.isfinite(raw1).all()
    assert np.abs(raw0.cpu().numpy() - raw1.cpu().numpy()).max() <= 2e-5 * max(1.0, float(raw0.abs().max()))
    assert np.abs(lat0.cpu().numpy() - lat1.cpu().numpy()).max() <= 5e-6
    _symbols_agree(q1.cpu().numpy(), lat0.cpu().numpy(), q0.cpu().numpy())
    a = ae.decode(q0, matmul="f32").cpu().numpy()
    b = ae.decode(q0, matmul="f16x2").cpu().numpy()
    assert np.isfinite(b).all()
    assert np.abs(a - b).max() <= 2e-6 * max(1.0, np.abs(a).max())
    if Kx == K:
        oae = ref_model.AE(K, k, d, L).eval()
        oae.load_state_dict(ae.state_dict())
        with torch.no_grad():
            olat = oae.encode(x.cpu())
            want = oae.decode(q0.cpu()).numpy()
        np.testing.assert_allclose(lat1.cpu().numpy(), olat.numpy(), rtol=0, atol=5e-5)
        np.testing.assert_allclose(b, want.reshape(b.shape), rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("Kx,P", [(256, 300), (512, 9)])
def test_f16x2_two_tile_pointnet_equals_one_tile_form_bit_for_bit(Kx, P, monkeypatch):
    """K a multiple of 256 runs PointNet's layers 1-3 with TWO point tiles per wave (csrc/encoder_fused_h2.hip, NT2: the weight stream
    once per 256 points, layer 2 in eight slices); PCCX_ENC_H2_NT=1 forces the one-tile form.  Every accumulator sees the same products
    in the same order, so raw latents, latents and symbols are IDENTICAL."""
    ae = _seeded_ae(Kx, Kx // 2)
    rng = np.random.default_rng(Kx + P)
    x = torch.from_numpy((rng.random((P, Kx, 3)).astype(np.float32) - 0.5) * np.exp2(rng.integers(-2, 3, size=(P, 1, 1))).astype(np.float32)).cuda()
    monkeypatch.delenv("PCCX_ENC_H2_NT", raising=False)
    a = ae.encode(x, sa_matmul="f16x2", pn_matmul="f16x2")
    monkeypatch.setenv("PCCX_ENC_H2_NT", "1")
    b = ae.encode(x, sa_matmul="f16x2", pn_matmul="f16x2")
    monkeypatch.delenv("PCCX_ENC_H2_NT", raising=False)
    c = ae.encode(x, sa_matmul="f16x2", pn_matmul="f16x2")
    for u, v, w_ in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w_)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_f16x2_over_randomly_scaled_weights(seed):
    """The operand scales come from interval bounds of whatever weights are packed.  Models whose layers are rescaled at random (each
    weight tensor by 2^[-3, 3], each bias by 0 ... 8, one layer's weights made sparse) must stay finite and agree with the exact-fp32
    kernels to the usual relative bars -- no layer may overflow fp16 or lose its low piece whatever the weights' magnitudes."""
    rng = np.random.default_rng(100 + seed)
    ae = models.AE(K, k, d, L)
    sd = ref_model.seeded_state_dict(ae, synth.AE_SEED + seed, last_gain=synth.AE_LAST_GAIN)
    for n in list(sd):
        if n.endswith("weight"):
            sd[n] = sd[n] * float(np.exp2(rng.uniform(-3, 3)))
        elif n.endswith("bias"):
            sd[n] = sd[n] * float(rng.uniform(0, 8))
    sp = sd["pn.mlp_Modules.2.0.weight"]
    sd["pn.mlp_Modules.2.0.weight"] = sp * torch.from_numpy((rng.random(tuple(sp.shape)) < 0.1).astype(np.float32))
    ae.load_state_dict(sd)
    ae.pack("cuda")
    x = torch.from_numpy((rng.random((40, K, 3)).astype(np.float32) - 0.5) * np.exp2(rng.integers(-4, 5, size=(40, 1, 1))).astype(np.float32)).cuda()
    raw0, _, _ = ae.encode(x, sa_matmul="f32", pn_matmul="f32")
    raw1, _, _ = ae.encode(x, sa_matmul="f16x2", pn_matmul="f16x2")
    raw3, _, _ = ae.encode(x, sa_matmul="bf16x3", pn_matmul="bf16x3")
    assert torch.isfinite(raw0).all() and torch.isfinite(raw1).all()
    scale = max(1e-30, float(raw0.abs().max()))
    e1, e3 = float((raw0 - raw1).abs().max()) / scale, float((raw0 - raw3).abs().max()) / scale
    assert e1 <= 2e-5 and e1 <= max(2e-6, 4.0 * e3), (e1, e3, scale)
    lq = torch.from_numpy(rng.integers(-3, 4, size=(40, d)).astype(np.float32)).cuda()
    a = ae.decode(lq, matmul="f32")
    b = ae.decode(lq, matmul="f16x2")
    c = ae.decode(lq, matmul="bf16x3")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    dscale = max(1e-30, float(a.abs().max()))
    d1, d3 = float((a - b).abs().max()) / dscale, float((a - c).abs().max()) / dscale
    assert d1 <= 2e-6 * max(1.0, 1.0 / dscale) and d1 <= max(1e-6, 4.0 * d3), (d1, d3, dscale)


def test_f16x2_at_the_largest_patch_and_without_the_fused_kernel(monkeypatch):
    """K = 1024: the f16x2 fused encoder still holds the patch (two fp16 weight planes leave the LDS the bf16x3 kernel lacks there):
    same bars against the exact-fp32 kernels as at K = 256, and its two forms agree bit for bit.  fused=False (ae.sa / ae.pn have no f16x2
    form of their own) runs the bf16x3 kernels: the same results as asking for them."""
    from pccx import _lib
    assert _lib.load().pccx_ae_encode_h2_fused_ok(1024) == 1 and _lib.load().pccx_ae_encode_b3_fused_ok(1024) == 0
    ae = _seeded_ae(1024, 512)
    rng = np.random.default_rng(5)
    x = torch.from_numpy((rng.random((2, 1024, 3)).astype(np.float32) - 0.5)).cuda()
    raw0, lat0, q0 = ae.encode(x, sa_matmul="f32", pn_matmul="f32")
    a = ae.encode(x, sa_matmul="f16x2", pn_matmul="f16x2")
    assert np.abs(raw0.cpu().numpy() - a[0].cpu().numpy()).max() <= 2e-5 * max(1.0, float(raw0.abs().max()))
    assert np.abs(lat0.cpu().numpy() - a[1].cpu().numpy()).max() <= 5e-6
    _symbols_agree(a[2].cpu().numpy(), lat0.cpu().numpy(), q0.cpu().numpy())
    monkeypatch.setenv("PCCX_ENC_H2_NT", "1")
    b = ae.encode(x, sa_matmul="f16x2", pn_matmul="f16x2")
    monkeypatch.delenv("PCCX_ENC_H2_NT", raising=False)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    ae2 = _seeded_ae(K, k)
    x2 = torch.from_numpy((rng.random((3, K, 3)).astype(np.float32) - 0.5)).cuda()
    c = ae2.encode(x2, sa_matmul="f16x2", pn_matmul="f16x2", fused=False)
    e = ae2.encode(x2, sa_matmul="bf16x3", pn_matmul="bf16x3", fused=False)
    assert all(torch.equal(u, v) for u, v in zip(c, e))


def test_integration_stub_of_the_f16x2_encoder(nets):
    """INTEGRATION.md, Option B: the ctypes stub a maintainer adds on the reference side for the batched analysis transform -- raw
    C ABI, weights packed on the host from state_dict tensors -- gives exactly what the host layer gives."""
    import ctypes
    from pccx import _lib
    ae = nets[0]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    _P = ctypes.c_void_p
    lib.pccx_last_error.restype = ctypes.c_char_p

    def _check(rc):
        if rc:
            raise RuntimeError(lib.pccx_last_error().decode())
    sd = ae.state_dict()
    w = lambda key: sd[key].reshape(sd[key].shape[0], -1).float().contiguous().cpu()
    keys = ["sa.conv0", "sa.conv1", "sa.conv2", "pn.mlp_Modules.0.0", "pn.mlp_Modules.1.0", "pn.mlp_Modules.2.0", "pn.mlp_Modules.3.0"]
    host = [t for key in keys for t in (w(key + ".weight"), sd[key + ".bias"].float().contiguous().cpu())]
    lib.pccx_ae_encoder_blob_floats.restype = lib.pccx_ae_encoder_h2_blob_floats.restype = ctypes.c_size_t
    enc = torch.zeros(lib.pccx_ae_encoder_blob_floats())
    _check(lib.pccx_pack_ae_encoder(*[_P(t.data_ptr()) for t in host], d, _P(enc.data_ptr())))
    h2 = torch.zeros(lib.pccx_ae_encoder_h2_blob_floats())
    _check(lib.pccx_pack_ae_encoder_h2(*[_P(t.data_ptr()) for t in host], d, _P(h2.data_ptr())))
    enc, h2 = enc.cuda(), h2.cuda()
    patches = torch.from_numpy(synth.patch_batch(K)).cuda().contiguous()
    P = patches.shape[0]
    raw, lat, q = (torch.empty(P, d, device="cuda") for _ in range(3))
    lib.pccx_ae_encode_h2_workspace_bytes.restype = ctypes.c_size_t
    ws = torch.empty(lib.pccx_ae_encode_h2_workspace_bytes(P, K), dtype=torch.uint8, device="cuda")
    _check(lib.pccx_ae_encode_h2_ws(_P(patches.data_ptr()), P, K, _P(enc.data_ptr()), _P(h2.data_ptr()), d, L, _P(raw.data_ptr()), _P(lat.data_ptr()),
                                    _P(q.data_ptr()), _P(ws.data_ptr()), _P(torch.cuda.current_stream().cuda_stream)))
    want = ae.encode(patches, sa_matmul="f16x2", pn_matmul="f16x2")
    assert torch.equal(raw, want[0]) and torch.equal(lat, want[1]) and torch.equal(q, want[2])


def test_every_mode_against_the_float64_oracle(nets):
    """How far each arithmetic is from the TRUE result: the oracle's modules evaluated in float64 on the same fp32 inputs and weights.
    The exact-fp32 MFMA kernels are themselves ~1e-6 away (fp32 accumulation); the split-operand modes must not be further than
    1.5 x that (measured: all three within 10 % of each other -- the accumulation, not the operand representation, dominates)."""
    ae, _, oae, _ = nets
    o64 = ref_model.AE(K, k, d, L).eval()
    o64.load_state_dict(oae.state_dict())
    o64 = o64.double()
    patches = synth.patch_batch(K)
    x = torch.from_numpy(patches).cuda()
    with torch.no_grad():
        lat64 = o64.encode(torch.from_numpy(patches).double()).numpy()
    err = {}
    for mode in ("f32", "bf16x3", "f16x2"):
        _, lat, q = ae.encode(x, sa_matmul=mode, pn_matmul=mode)
        err[mode] = np.abs(lat.cpu().numpy().astype(np.float64) - lat64)
    print("latent error against float64, max / rms:", {m: (float(e.max()), float(np.sqrt((e ** 2).mean()))) for m, e in err.items()})
    for mode in ("bf16x3", "f16x2"):
        assert err[mode].max() <= 1.5 * err["f32"].max() + 1e-7, (mode, err[mode].max(), err["f32"].max())
        assert np.sqrt((err[mode] ** 2).mean()) <= 1.5 * np.sqrt((err["f32"] ** 2).mean()) + 1e-8
    lq = torch.from_numpy(synth.latent_case(2, d, L))
    with torch.no_grad():
        dec64 = o64.decode(lq.double()).numpy()
    derr = {}
    for mode in ("f32", "bf16x3", "f16x2"):
        out = ae.decode(lq.cuda(), matmul=mode).cpu().numpy().astype(np.float64)
        derr[mode] = np.abs(out - dec64.reshape(out.shape))
    print("decoder error against float64, max / rms:", {m: (float(e.max()), float(np.sqrt((e ** 2).mean()))) for m, e in derr.items()})
    for mode in ("bf16x3", "f16x2"):
        assert derr[mode].max() <= 1.5 * derr["f32"].max() + 1e-8, (mode, derr[mode].max(), derr["f32"].max())
        assert np.sqrt((derr[mode] ** 2).mean()) <= 1.5 * np.sqrt((derr["f32"] ** 2).mean()) + 1e-9


@pytest.mark.parametrize("kx,P", [(128, 700), (32, 37), (256, 3)])
def test_f16x2_decoder_four_tile_form_equals_two_tile_form_bit_for_bit(kx, P, monkeypatch):
    """dec_main_h2_kernel<4> (four patch tiles per wave in the GEMM, inv_mlp in two batches from the tail's second copy in the stream;
    the default) against <2> (PCCX_DEC_H2_NT=2): every accumulator sees the same products in the same order, so the outputs are
    IDENTICAL; P = 700 leaves the last workgroup with clamped tiles, P = 3 all but one wave."""
    ae = _seeded_ae(2 * kx, kx)
    rng = np.random.default_rng(kx + P)
    lq = torch.from_numpy(rng.integers(-3, 4, size=(P, d)).astype(np.float32) * np.exp2(rng.integers(-1, 3, size=(P, 1))).astype(np.float32)).cuda()
    monkeypatch.delenv("PCCX_DEC_H2_NT", raising=False)
    a = ae.decode(lq, matmul="f16x2")
    monkeypatch.setenv("PCCX_DEC_H2_NT", "2")
    b = ae.decode(lq, matmul="f16x2")
    monkeypatch.delenv("PCCX_DEC_H2_NT", raising=False)
    c = ae.decode(lq, matmul="f16x2")
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)
    ref = ae.decode(lq, matmul="f32")
    assert float((a - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("P", [1, 17, 129, 257])
def test_bf16x3_decoder_four_tile_form_equals_two_tile_form_bit_for_bit(P, monkeypatch):
    """dec_main_kernel_b3<4> (PCCX_DEC_NT=4: four patch tiles per wave, one wave per SIMD) against <2> (the default): both run the same
    k loop over the same operands and every accumulator sees the same products in the same order, so the outputs are IDENTICAL, as
    patches and as the reassembled cloud.  P = 1 and 17 leave all but one wave on clamped tiles, 129 starts a second workgroup of the
    two-tile form inside the first of the four-tile form, 257 a second one of the four-tile form."""
    kx = 32
    ae = _seeded_ae(2 * kx, kx)
    rng = np.random.default_rng(100 + P)
    lq = torch.from_numpy(rng.integers(-3, 4, size=(P, d)).astype(np.float32)).cuda()
    centres = torch.from_numpy(((rng.integers(0, 128, size=(1, P, 3)) + 0.5) / 128).astype(np.float32)).cuda()
    center = torch.from_numpy(rng.normal(size=(1, 3)).astype(np.float32)).cuda()
    longest = torch.from_numpy((1 + rng.random(1)).astype(np.float32)).cuda()
    cloud = dict(centres=centres, center=center, longest=longest, S=P, scale=float((P * kx / 1024) ** (1 / 3)))
    monkeypatch.delenv("PCCX_DEC_NT", raising=False)
    a, pa = ae.decode(lq, matmul="bf16x3"), ae.decode(lq, matmul="bf16x3", **cloud)
    monkeypatch.setenv("PCCX_DEC_NT", "4")
    b, pb = ae.decode(lq, matmul="bf16x3"), ae.decode(lq, matmul="bf16x3", **cloud)
    monkeypatch.delenv("PCCX_DEC_NT", raising=False)
    c = ae.decode(lq, matmul="bf16x3")
    assert a.shape == (P, kx, 3) and pa.shape == (1, P * kx, 3)
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)
    assert torch.isfinite(pa).all() and torch.equal(pa, pb)


@pytest.mark.parametrize("scale", [1e-6, 1e-3, 1.0, 0.99999994, 2.0, 37.0, 3000.0, 1e6])
def test_f16x2_per_patch_normalisation_over_input_magnitudes(scale):
    """fp16 has five exponent bits; the f16x2 kernels bring every operand into range with exact power-of-two scales, one of them
    per patch from the data (largest |coordinate| for the encoder; largest head activation or |latent| for the decoder).  Patches
    and latents of very different magnitudes in ONE launch (each row scaled by its own factor around `scale`, one row all-zero,
    one with a single far outlier) must stay finite and agree with the exact-fp32 kernels as closely as at scale 1."""
    ae = _seeded_ae(K, k, bias_gain=4.0)                               # large biases: the scaled-bias path carries weight
    rng = np.random.default_rng(11)
    P = 48
    x = (rng.random((P, K, 3)).astype(np.float32) - 0.5)
    row = (scale * np.exp2(rng.integers(-3, 4, size=(P, 1, 1)))).astype(np.float32)
    x = x * row
    x[1] = 0.0                                                       # degenerate patch: every point at the centre
    x[2, 5] = 50.0 * row[2, 0]                                        # one far outlier sets the patch's scale
    x = torch.from_numpy(x).cuda()
    raw0, lat0, q0 = ae.encode(x, sa_matmul="f32", pn_matmul="f32")
    raw1, lat1, q1 = ae.encode(x, sa_matmul="f16x2", pn_matmul="f16x2")
    raw3, lat3, _ = ae.encode(x, sa_matmul="bf16x3", pn_matmul="bf16x3")
    assert torch.isfinite(raw1).all()
    assert np.abs(raw0.cpu().numpy() - raw1.cpu().numpy()).max() <= 2e-5 * max(1.0, float(raw0.abs().max()))
    # latent = (L - 0.2) sigmoid(raw) - const, so |d latent| <= (L - 0.2) / 4 |d raw|: with biases four times the usual ones and
    # coordinates up to 1e6 the pre-sigmoid values reach hundreds, and the latent bar follows the raw bar above instead of being the
    # 5e-6 of the unit-scale tests; the f16x2 kernel is also held to within 3 x of what the bf16x3 kernel shows on the same input
    e1 = np.abs(lat0.cpu().numpy() - lat1.cpu().numpy()).max()
    e3 = np.abs(lat0.cpu().numpy() - lat3.cpu().numpy()).max()
    assert e1 <= (L - 0.2) / 4 * 2e-5 * max(1.0, float(raw0.abs().max())) and e1 <= max(5e-6, 3.0 * e3), (e1, e3, float(raw0.abs().max()))
    _symbols_agree(q1.cpu().numpy(), lat0.cpu().numpy(), q0.cpu().numpy())
    lq = rng.integers(-3, 4, size=(P, d)).astype(np.float32) * row[:, 0]
    lq[1] = 0.0
    lq = torch.from_numpy(lq).cuda()
    a = ae.decode(lq, matmul="f32").cpu().numpy()
    b = ae.decode(lq, matmul="f16x2").cpu().numpy()
    assert np.isfinite(b).all()
    per = np.abs(a).max(axis=(1, 2), keepdims=True)
    assert (np.abs(a - b) <= 2e-6 * np.maximum(per, 1.0)).all(), float((np.abs(a - b) / np.maximum(per, 1.0)).max())


@pytest.mark.parametrize("Kx,P", [(256, 7), (64, 5), (16, 3), (48, 2), (512, 3), (1024, 1)])
def test_fused_encoder_kernel_equals_the_two_kernel_path_bit_for_bit(Kx, P):
    """pccx_ae_encode_b3 (SetAbstraction + PointNet + quantiser in one kernel, the feature map handed over inside the CU)
    against pccx_sa_forward_b3 + pccx_pn_forward_b3 through the HBM feature map: the same products in the same order, so
    raw latents, latents and symbols are IDENTICAL.  K = 48 leaves five of the eight waves without a tile; K = 1024 does
    not fit the fused kernel's LDS budget and must fall back to the two kernels transparently."""
    from pccx import _lib
    ae = models.AE(Kx, Kx // 2, d, L)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    ae.pack("cuda")
    assert bool(_lib.load().pccx_ae_encode_b3_fused_ok(Kx)) == (Kx <= 512)
    rng = np.random.default_rng(Kx * 31 + P)
    x = torch.from_numpy((rng.random((P, Kx, 3)).astype(np.float32) - 0.5)).cuda()
    x[0, : Kx // 2] = x[0, Kx // 2:]                                  # duplicated points: the tie path of the in-patch kNN
    a = ae.encode(x, sa_matmul="bf16x3", pn_matmul="bf16x3", fused=True)
    b = ae.encode(x, sa_matmul="bf16x3", pn_matmul="bf16x3", fused=False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # and twice in a row on a big launch (ring / staging reuse across passes and patches)
    if Kx == 256:
        xb = torch.from_numpy((rng.random((600, Kx, 3)).astype(np.float32) - 0.5)).cuda()
        a = ae.encode(xb, sa_matmul="bf16x3", pn_matmul="bf16x3", fused=True)
        b = ae.encode(xb, sa_matmul="bf16x3", pn_matmul="bf16x3", fused=False)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("Kx", [256, 64, 16, 48, 512, 1024])
def test_patch_knn16_table_equals_the_oracle_sets_and_feeds_the_fused_encoder(Kx):
    """pccx_patch_knn16 (csrc/patch_knn.hip: the in-patch 16-NN of pn_kit.py:186-190 as its own kernel) against orc_knn on
    patches that hit both sides of its boundary test -- a lattice (exact ties), a jittered shell (near-ties in the dropped
    distance bits), duplicated points, random -- compared as SETS per point (a max-pool follows; the row order is unspecified);
    and pccx_ae_encode_b3_ws (table from that kernel) against pccx_ae_encode_b3 (selection inside the encoder): bit-identical."""
    from oracle import cport
    from pccx import _lib
    lib = _lib.load()
    rng = np.random.default_rng(Kx)
    n = Kx
    side = int(np.ceil(n ** (1 / 3)))
    lattice = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)
    lattice = ((lattice[rng.permutation(len(lattice))[:n]] - side / 2) * 0.05).astype(np.float32)
    dirs = rng.normal(size=(n - 1, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    shell = np.concatenate([np.zeros((1, 3)), dirs * (0.3 * (1.0 + rng.integers(-40, 41, size=(n - 1, 1)) * 2.0 ** -24))]).astype(np.float32)
    dup = rng.uniform(-0.4, 0.4, size=(n // 2, 3)).astype(np.float32)
    dup = np.concatenate([dup, dup])[rng.permutation(n)]
    rand = rng.uniform(-0.5, 0.5, size=(n, 3)).astype(np.float32)
    patches = np.stack([lattice, shell, dup, rand])
    x = torch.from_numpy(patches).cuda()
    P = x.shape[0]
    ib = lib.pccx_patch_knn16_index_bytes(Kx)
    assert ib == (1 if Kx <= 256 else 2) and lib.pccx_patch_knn16_bytes(P, Kx) == P * Kx * 16 * ib
    tab = torch.zeros(P * Kx * 16, dtype=torch.uint8 if ib == 1 else torch.int16, device="cuda")
    _lib.call("pccx_patch_knn16", x.data_ptr(), P, Kx, tab.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got = tab.cpu().numpy().astype(np.int64).reshape(P, Kx, 16)
    for p_ in range(P):
        _, want = cport.knn(patches[p_], patches[p_], 16)
        assert np.array_equal(np.sort(got[p_], axis=1), np.sort(want, axis=1)), f"patch {p_}: neighbour sets differ from orc_knn"
    if lib.pccx_ae_encode_b3_fused_ok(Kx):
        ae = models.AE(Kx, Kx // 2, d, L)
        ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
        ae.pack("cuda")
        enc, _ = ae._blobs(x.device)
        st = torch.cuda.current_stream().cuda_stream
        a = [torch.zeros(P, d, device="cuda") for _ in range(3)]
        b = [torch.zeros(P, d, device="cuda") for _ in range(3)]
        _lib.call("pccx_ae_encode_b3", x.data_ptr(), P, Kx, enc.data_ptr(), ae._sa_b3_blob(x.device).data_ptr(), ae._pn_b3_blob(x.device).data_ptr(),
                  d, L, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), st)
        _lib.call("pccx_ae_encode_b3_ws", x.data_ptr(), P, Kx, enc.data_ptr(), ae._sa_b3_blob(x.device).data_ptr(), ae._pn_b3_blob(x.device).data_ptr(),
                  d, L, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), tab.data_ptr(), st)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("dx,Lx", [(20, 9), (32, 7), (16, 9)])
def test_bottleneck_widths_beyond_the_fused_kernels_take_the_generic_layers(dx, Lx, matmul_mode):
    """compress.py:30-34 accepts any --d / --L.  The fused PointNet / decoder cover d <= 16 and the fused probability model
    d * L <= 128; beyond that models.AE / ConditionalProbabilityModel run the same statements through the generic layer kernels
    (encode_generic / decode_generic / _run_generic + pccx_softmax_cdf + pccx_reassemble).  Against the oracle modules at the
    tolerances of the fused path: latents 5e-5, symbols equal away from rounding boundaries, decoder output 2e-5, pmf 2e-6, integer
    CDF within +-1; and a whole compress -> decompress of one cloud reproduces the oracle's reconstruction."""
    from oracle import ref_pipeline
    from pccx import codec
    from pccx import synth as cloud_synth
    Kx, kx = 64, 32
    ae = models.AE(Kx, kx, dx, Lx)
    ae.load_state_dict(ref_model.seeded_state_dict(ae, synth.AE_SEED, last_gain=synth.AE_LAST_GAIN))
    prob = models.ConditionalProbabilityModel(Lx, dx)
    prob.load_state_dict(ref_model.seeded_state_dict(prob, synth.PROB_SEED, gain=synth.PROB_GAIN))
    oae = ref_model.AE(Kx, kx, dx, Lx).eval()
    oae.load_state_dict(ae.state_dict())
    oprob = ref_model.ConditionalProbabilityModel(Lx, dx).eval()
    oprob.load_state_dict(prob.state_dict())
    ae.pack("cuda")
    prob.pack("cuda")
    assert ae.fused_d == (dx <= 16) and not prob.fused_ok(64)
    rng = np.random.default_rng(dx * 100 + Lx)
    x = (rng.random((7, Kx, 3)).astype(np.float32) - 0.5)
    raw, latent, q = ae.encode(torch.from_numpy(x).cuda())
    with torch.no_grad():
        olat = oae.encode(torch.from_numpy(x))
        oq = olat.round()
        odec = oae.decode(oq)
    np.testing.assert_allclose(latent.cpu().numpy(), olat.numpy(), rtol=0, atol=5e-5)
    _symbols_agree(q.cpu().numpy(), olat.numpy(), oq.numpy())
    np.testing.assert_allclose(ae.decode(oq.cuda()).cpu().numpy(), odec.numpy(), rtol=1e-4, atol=2e-5)
    cent = ((rng.integers(0, 64, size=(2, 64, 3)) + 0.5) / 64).astype(np.float32)
    r = prob.run(torch.from_numpy(cent).cuda(), ("pmf", "cdf", "cdf_int"))
    with torch.no_grad():
        opmf = oprob(torch.from_numpy(cent))
    np.testing.assert_allclose(r["pmf"].cpu().numpy(), opmf.numpy(), rtol=0, atol=2e-6)
    want = ref_model.cdf_float_to_int(ref_model.pmf_to_cdf(opmf))
    diff = ((r["cdf_int"].cpu().numpy().astype(np.int64) - want.astype(np.int64) + 32768) % 65536) - 32768
    assert np.abs(diff).max() <= 1
    # the whole path on one cloud (N = 2048, K = 64: S = 64 patches), against the oracle loop
    pc = cloud_synth.cad_cloud(77, 2048)
    cd = codec.Codec(ae, prob, K=Kx)
    comp = cd.compress(torch.from_numpy(pc)[None].cuda(), [5], keep_extras=True)
    out = cd.decompress(comp)
    o, _ = ref_pipeline.compress_one(pc, oae, oprob, 5, K=Kx)
    s_, p_, c_ = comp.files(0)
    assert s_ == o["s"] and c_ == o["c"]
    qg = comp.extras["latent_q"].view(64, dx).cpu().numpy()
    want_pc, _ = ref_pipeline.decompress_one(s_, p_, c_, oae, oprob, latent_q_override=qg.copy())
    np.testing.assert_allclose(out[0].cpu().numpy(), want_pc, rtol=0, atol=2e-5 * float(comp.c[0, 3]))
