"""INTEGRATION.md section 2's claim: `MI355WanAttnProcessor` / `MI355CogVideoXAttnProcessor` installed with `set_processor`
on an `Attention` carrying the reference's parameters are called through its `forward` (kwarg filtering by signature,
reference attention_processor.py:556-600) and return what the reference's own `WanAttnProcessor2_0` /
`CogVideoXAttnProcessor2_0` returned on the same parameters and inputs.

The reference's side is recorded in tests/golden/reference_plugin.npz (tools/golden/make_golden.py::gen_plugin runs the
reference's own `Attention` and processors on CPU): parameters under the reference's names, inputs, rotary tables, outputs.
Here the parameters load into `frameino_amd.attention_processor.Attention` strictly by those names.  No GPU here: the
processors' kernel front end (`frameino_amd.ops`) is swapped for tests/cpu_ops.py, so what is checked is the PROTOCOL --
attribute names read off `attn`, argument passing, output shapes / tuple order -- and the processor body's arithmetic
structure; the kernels themselves are the -m gpu tests' business."""
import pytest
import torch


@pytest.fixture()
def ref_modules(monkeypatch, golden):
    from tests import cpu_ops
    import frameino_amd.attention_processor as ap
    monkeypatch.setattr(ap, "ops", cpu_ops)
    monkeypatch.setattr(cpu_ops, "headnorm_rope_", _headnorm_rope_, raising=False)
    _, _, rec = golden("reference_plugin")
    return ap, rec


def _state_dict(rec, prefix):
    return {k[len(prefix):]: v for k, v in rec.items() if k.startswith(prefix)}


def _headnorm_rope_(x, heads, head_dim, weight, bias, eps, cos=None, sin=None, rope_row0=0):
    """CPU contract of fino_headnorm_rope: per-head LayerNorm + adjacent-pair RoPE on rows >= rope_row0, in place."""
    import torch.nn.functional as F
    b, rows, _ = x.shape
    y = x.reshape(b, rows, heads, head_dim).float()
    if weight is not None:
        y = F.layer_norm(y, (head_dim,), weight.float(), bias.float(), eps)
    if cos is not None:
        v = y[:, rope_row0:]
        xr, xi = v.reshape(*v.shape[:-1], -1, 2).unbind(-1)
        rot = torch.stack([-xi, xr], dim=-1).flatten(3)
        y[:, rope_row0:] = v * cos[None, :, None, :] + rot * sin[None, :, None, :]
    x.copy_(y.reshape(b, rows, heads * head_dim).to(x.dtype))
    return x


def test_wan_processor_on_the_references_attention(ref_modules):
    ap, rec = ref_modules
    heads, dh = 2, 24
    d = heads * dh
    for cross in (False, True):
        pre = f"wan{int(cross)}/"
        attn = ap.Attention(query_dim=d, heads=heads, kv_heads=heads, dim_head=dh, qk_norm="rms_norm_across_heads",
                            eps=1e-6, bias=True, cross_attention_dim=None, out_bias=True).eval()
        attn.load_state_dict(_state_dict(rec, pre + "sd/"), strict=True)      # the reference's parameter names, all of them
        x, ref = rec[pre + "x"], rec[pre + "out"]
        ctx = rec[pre + "ctx"] if cross else None
        rot = None if cross else (rec[pre + "rot_cos"], rec[pre + "rot_sin"])
        with torch.no_grad():
            attn.set_processor(ap.MI355WanAttnProcessor())                  # the plugin call a maintainer makes
            assert isinstance(attn.get_processor(), ap.MI355WanAttnProcessor)
            out = attn(x, encoder_hidden_states=ctx, rotary_emb=rot, some_unknown_kwarg=1)     # filtered by signature
        torch.testing.assert_close(out, ref, atol=2e-5, rtol=2e-5)


def test_cogvideox_processors_on_the_references_attention(ref_modules):
    ap, rec = ref_modules
    heads, dh = 2, 16
    d = heads * dh
    attn = ap.Attention(query_dim=d, dim_head=dh, heads=heads, qk_norm="layer_norm", eps=1e-6, bias=True,
                        out_bias=True).eval()
    attn.load_state_dict(_state_dict(rec, "cog/sd/"), strict=True)
    txt, vid = rec["cog/txt"], rec["cog/vid"]
    cos, sin = rec["cog/cos"], rec["cog/sin"]
    rh, re = rec["cog/out_hidden"], rec["cog/out_encoder"]
    with torch.no_grad():
        attn.set_processor(ap.MI355CogVideoXAttnProcessor())
        oh, oe = attn(vid, encoder_hidden_states=txt, image_rotary_emb=(cos, sin))
        torch.testing.assert_close(oh, rh, atol=2e-5, rtol=2e-5)
        torch.testing.assert_close(oe, re, atol=2e-5, rtol=2e-5)
        attn.fuse_projections()                                             # the reference's fuse (:769-820)
        attn.set_processor(ap.MI355FusedCogVideoXAttnProcessor())
        fh, fe = attn(vid, encoder_hidden_states=txt, image_rotary_emb=(cos, sin))
        torch.testing.assert_close(fh, rh, atol=2e-5, rtol=2e-5)
        torch.testing.assert_close(fe, re, atol=2e-5, rtol=2e-5)


def test_reference_tiling_raises_on_the_wan22_vae_and_the_mirror_says_so(ref_modules):
    """frameino_amd/autoencoder_kl_wan.py::enable_tiling returns the un-tiled result because the REFERENCE's tiled paths
    (architecture/autoencoder_kl_wan.py:1270-1397) produce none on the Wan2.2 VAE (patch_size=2, is_residual=True): tiled_encode
    feeds un-patchified tiles to a 12-channel conv_in, tiled_decode drops first_chunk.  Both were recorded on the reference's own
    class (and its un-tiled decode works); the mirror's one-time warning is checked next to them."""
    import warnings
    _, rec = ref_modules
    assert "12 channels" in str(rec["tiled_encode_error"]) and str(rec["tiled_encode_error"]).startswith("RuntimeError")
    assert "must match the size" in str(rec["tiled_decode_error"]) and str(rec["tiled_decode_error"]).startswith("RuntimeError")
    assert tuple(rec["untiled_decode_shape"].tolist()) == (1, 3, 5, 64, 96)
    cfg = dict(base_dim=8, decoder_base_dim=16, z_dim=4, dim_mult=[1, 2, 4, 4], num_res_blocks=1, attn_scales=[],
               temperal_downsample=[False, True, True], dropout=0.0, latents_mean=[0.0] * 4, latents_std=[1.0] * 4,
               is_residual=True, in_channels=12, out_channels=12, patch_size=2, scale_factor_temporal=4, scale_factor_spatial=16)
    from frameino_amd.autoencoder_kl_wan import AutoencoderKLWan
    AutoencoderKLWan._warned_tiling = False
    mine = AutoencoderKLWan(**cfg)
    with pytest.warns(RuntimeWarning, match="UN-TILED"):
        mine.enable_tiling(tile_sample_min_height=32)
    assert mine.use_tiling and mine.tile_sample_min_height == 32 and mine.decode_chunk_frames == 8
    with warnings.catch_warnings():
        warnings.simplefilter("error")                         # once per process
        mine.enable_tiling()
    mine.disable_tiling()
    assert not mine.use_tiling and mine.decode_chunk_frames == "auto"
