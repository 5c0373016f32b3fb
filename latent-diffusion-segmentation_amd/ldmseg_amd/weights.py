"""State-dict schemas and a deterministic weight generator.

The schemas enumerate the exact key set / shapes a reference checkpoint holds:
  * UNet: ``data['unet']`` of ldmseg.pt
    (/root/reference/ldmseg/trainers/trainers_ldm_cond.py:1791-1814) - the
    diffusers SD-1.x UNet2DConditionModel key set after
    ``remove_cross_attention`` (unet.py:83-105) and ``modify_encoder``
    (unet.py:178-233).  Validated by the known totals: 859,520,964 params /
    686 tensors (vanilla) and 815,556,484 / 574 (12-ch, no cross-attn).
  * seg-VAE: ``GeneralVAESeg.state_dict()`` (vae.py:123-244), 34 tensors,
    2,023,208 params for base.yaml:14-33.

No pretrained weights exist offline, so benchmarks and tests run on weights
drawn by ``generate`` (per-tensor seed = crc32(key) ^ seed).  Matrices/filters
are U(+-sqrt(3/fan_in)) (variance preserving, so activations stay O(1) through
38 blocks and softmax is non-trivial); biases U(+-0.05); norm gains 1 +- 0.1.
"""
import zlib
from collections import OrderedDict

import torch

BLOCK_OUT = (320, 640, 1280, 1280)
TIME_DIM = 1280
CROSS_DIM = 768
HID_PROJ_IN = 1024          # CLIP-L/14 patch features (image_descriptors: clip_image)


def hid_proj_schema():
    """encoder_hid_proj = Linear(1024, 768): the optional projection of a cross-attention UNet (unet.py:121-122)."""
    return OrderedDict([("encoder_hid_proj.weight", (CROSS_DIM, HID_PROJ_IN)), ("encoder_hid_proj.bias", (CROSS_DIM,))])


def separate_encoder_schema(add_adaptor=False):
    """The extra tensors of ``modify_encoder(separate_encoder=True)`` (unet.py:42-63): ``conv_in_img`` and
    ``down_blocks_additional`` - deep copies of the 4-channel ``conv_in`` and of ``down_blocks`` after
    ``remove_cross_attention`` (main_ldm.py:155-159 runs it first) - and, with ``add_adaptor``, one 3x3 conv C -> C per level.
    Together with ``unet_schema(4)``: 1,049,661,444 parameters in 780 tensors, 1,083,764,164 in 788 with the adaptors."""
    base = unet_schema(4, False)
    sd = OrderedDict()
    sd["conv_in_img.weight"] = base["conv_in.weight"]
    sd["conv_in_img.bias"] = base["conv_in.bias"]
    for k, shp in base.items():
        if k.startswith("down_blocks."):
            sd["down_blocks_additional." + k[len("down_blocks."):]] = shp
    if add_adaptor:
        for i, c in enumerate(BLOCK_OUT):
            sd[f"adaptor_layers.{i}.weight"] = (c, c, 3, 3)
            sd[f"adaptor_layers.{i}.bias"] = (c,)
    return sd


def separate_conv_schema():
    """``conv_in_seg`` of ``modify_encoder(separate_conv=True)`` (unet.py:140-173): a second 4-channel conv_in for the
    segmentation half; ``conv_in`` itself then reads the image half."""
    return OrderedDict([("conv_in_seg.weight", (BLOCK_OUT[0], 4, 3, 3)), ("conv_in_seg.bias", (BLOCK_OUT[0],))])


def _resnet(sd, p, cin, cout):
    sd[p + "norm1.weight"] = (cin,)
    sd[p + "norm1.bias"] = (cin,)
    sd[p + "conv1.weight"] = (cout, cin, 3, 3)
    sd[p + "conv1.bias"] = (cout,)
    sd[p + "time_emb_proj.weight"] = (cout, TIME_DIM)
    sd[p + "time_emb_proj.bias"] = (cout,)
    sd[p + "norm2.weight"] = (cout,)
    sd[p + "norm2.bias"] = (cout,)
    sd[p + "conv2.weight"] = (cout, cout, 3, 3)
    sd[p + "conv2.bias"] = (cout,)
    if cin != cout:
        sd[p + "conv_shortcut.weight"] = (cout, cin, 1, 1)
        sd[p + "conv_shortcut.bias"] = (cout,)


def _transformer(sd, p, c, cross):
    sd[p + "norm.weight"] = (c,)
    sd[p + "norm.bias"] = (c,)
    sd[p + "proj_in.weight"] = (c, c, 1, 1)
    sd[p + "proj_in.bias"] = (c,)
    b = p + "transformer_blocks.0."
    sd[b + "norm1.weight"] = (c,)
    sd[b + "norm1.bias"] = (c,)
    for n in ("to_q", "to_k", "to_v"):
        sd[b + f"attn1.{n}.weight"] = (c, c)
    sd[b + "attn1.to_out.0.weight"] = (c, c)
    sd[b + "attn1.to_out.0.bias"] = (c,)
    if cross:
        sd[b + "norm2.weight"] = (c,)
        sd[b + "norm2.bias"] = (c,)
        sd[b + "attn2.to_q.weight"] = (c, c)
        sd[b + "attn2.to_k.weight"] = (c, CROSS_DIM)
        sd[b + "attn2.to_v.weight"] = (c, CROSS_DIM)
        sd[b + "attn2.to_out.0.weight"] = (c, c)
        sd[b + "attn2.to_out.0.bias"] = (c,)
    sd[b + "norm3.weight"] = (c,)
    sd[b + "norm3.bias"] = (c,)
    sd[b + "ff.net.0.proj.weight"] = (8 * c, c)
    sd[b + "ff.net.0.proj.bias"] = (8 * c,)
    sd[b + "ff.net.2.weight"] = (c, 4 * c)
    sd[b + "ff.net.2.bias"] = (c,)
    sd[p + "proj_out.weight"] = (c, c, 1, 1)
    sd[p + "proj_out.bias"] = (c,)


def unet_schema(in_channels=12, cross_attention=False):
    """Ordered key -> shape for the SD-1.x UNet as LDMSeg instantiates it."""
    sd = OrderedDict()
    sd["conv_in.weight"] = (BLOCK_OUT[0], in_channels, 3, 3)
    sd["conv_in.bias"] = (BLOCK_OUT[0],)
    sd["time_embedding.linear_1.weight"] = (TIME_DIM, BLOCK_OUT[0])
    sd["time_embedding.linear_1.bias"] = (TIME_DIM,)
    sd["time_embedding.linear_2.weight"] = (TIME_DIM, TIME_DIM)
    sd["time_embedding.linear_2.bias"] = (TIME_DIM,)
    skip_ch = [BLOCK_OUT[0]]
    c = BLOCK_OUT[0]
    for i, co in enumerate(BLOCK_OUT):
        for j in range(2):
            _resnet(sd, f"down_blocks.{i}.resnets.{j}.", c, co)
            c = co
            if i < 3:
                _transformer(sd, f"down_blocks.{i}.attentions.{j}.", c, cross_attention)
            skip_ch.append(c)
        if i < 3:
            sd[f"down_blocks.{i}.downsamplers.0.conv.weight"] = (c, c, 3, 3)
            sd[f"down_blocks.{i}.downsamplers.0.conv.bias"] = (c,)
            skip_ch.append(c)
    _resnet(sd, "mid_block.resnets.0.", c, c)
    _transformer(sd, "mid_block.attentions.0.", c, cross_attention)
    _resnet(sd, "mid_block.resnets.1.", c, c)
    for i, co in enumerate(reversed(BLOCK_OUT)):
        for j in range(3):
            _resnet(sd, f"up_blocks.{i}.resnets.{j}.", c + skip_ch.pop(), co)
            c = co
            if i > 0:
                _transformer(sd, f"up_blocks.{i}.attentions.{j}.", c, cross_attention)
        if i < 3:
            sd[f"up_blocks.{i}.upsamplers.0.conv.weight"] = (c, c, 3, 3)
            sd[f"up_blocks.{i}.upsamplers.0.conv.bias"] = (c,)
    sd["conv_norm_out.weight"] = (c,)
    sd["conv_norm_out.bias"] = (c,)
    sd["conv_out.weight"] = (4, c, 3, 3)
    sd["conv_out.bias"] = (4,)
    return sd


def vae_schema(in_channels=7, int_channels=256, out_channels=128,
               block_out_channels=(32, 64, 128, 256), latent_channels=4,
               num_latents=2, num_upscalers=2, upscale_channels=256):
    """Ordered key -> shape of GeneralVAESeg (gaussian, num_mid_blocks=0)."""
    sd = OrderedDict()

    def conv(name, co, ci, k=3):
        sd[name + ".weight"] = (co, ci, k, k)
        sd[name + ".bias"] = (co,)

    boc = tuple(block_out_channels)
    conv("encoder.0", boc[0], in_channels)
    idx = 2
    for i in range(len(boc) - 1):
        conv(f"encoder.{idx}", boc[i], boc[i])
        conv(f"encoder.{idx + 1}", boc[i + 1], boc[i])
        idx += 3
    conv(f"encoder.{idx}", int_channels, boc[-1])          # 11
    sd[f"encoder.{idx + 2}.weight"] = (int_channels,)      # 13 GroupNorm
    sd[f"encoder.{idx + 2}.bias"] = (int_channels,)
    conv(f"encoder.{idx + 4}", latent_channels * num_latents, int_channels)  # 15
    conv("decoder.0", int_channels, latent_channels)
    idx = 2
    cin = int_channels
    for _ in range(num_upscalers):
        sd[f"decoder.{idx}.weight"] = (cin, upscale_channels, 2, 2)   # ConvTranspose2d [in,out,kh,kw]
        sd[f"decoder.{idx}.bias"] = (upscale_channels,)
        sd[f"decoder.{idx + 1}.weight"] = (upscale_channels,)         # LayerNorm2d
        sd[f"decoder.{idx + 1}.bias"] = (upscale_channels,)
        cin = upscale_channels
        idx += 3
    sd[f"decoder.{idx}.weight"] = (upscale_channels,)                  # GroupNorm
    sd[f"decoder.{idx}.bias"] = (upscale_channels,)
    conv(f"decoder.{idx + 2}", out_channels, upscale_channels)
    return sd


def vae_image_schema(old_attention_names=True):
    """Ordered key -> shape of the encoder half of the SD-1.x AutoencoderKL (GeneralVAEImage with the decoder
    removed, tools/main_ldm.py:137-139) + quant_conv.  diffusers 0.16.1 names the attention projections
    query/key/value/proj_attn; later releases to_q/to_k/to_v/to_out.0."""
    sd = OrderedDict()

    def conv(name, co, ci, k=3):
        sd[name + ".weight"] = (co, ci, k, k)
        sd[name + ".bias"] = (co,)

    def norm(name, c):
        sd[name + ".weight"] = (c,)
        sd[name + ".bias"] = (c,)

    def resnet(p, ci, co):
        norm(p + "norm1", ci)
        conv(p + "conv1", co, ci)
        norm(p + "norm2", co)
        conv(p + "conv2", co, co)
        if ci != co:
            conv(p + "conv_shortcut", co, ci, 1)

    ch = (128, 256, 512, 512)
    conv("encoder.conv_in", ch[0], 3)
    cin = ch[0]
    for i, co in enumerate(ch):
        for j in range(2):
            resnet(f"encoder.down_blocks.{i}.resnets.{j}.", cin, co)
            cin = co
        if i < 3:
            conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", co, co)
    resnet("encoder.mid_block.resnets.0.", 512, 512)
    ap = "encoder.mid_block.attentions.0."
    norm(ap + "group_norm", 512)
    for nm in (("query", "key", "value", "proj_attn") if old_attention_names else ("to_q", "to_k", "to_v", "to_out.0")):
        sd[ap + nm + ".weight"] = (512, 512)
        sd[ap + nm + ".bias"] = (512,)
    resnet("encoder.mid_block.resnets.1.", 512, 512)
    norm("encoder.conv_norm_out", 512)
    conv("encoder.conv_out", 8, 512)
    conv("quant_conv", 8, 8, 1)
    return sd


VAE_IMAGE_NORM_KEYS = ("encoder.mid_block.attentions.0.group_norm.weight", "encoder.mid_block.attentions.0.group_norm.bias")


def clip_vision_schema(hidden=1024, intermediate=4096, layers=24, heads=16, image=224, patch=14, projection_dim=0):
    """Ordered key -> shape of transformers' CLIPVisionModel.state_dict() without the ``vision_model.`` prefix (the image
    descriptor of image_descriptors clip_image, ldmseg/models/descriptors.py:15-56), plus
    ``visual_projection.weight`` of CLIPVisionModelWithProjection when projection_dim > 0 (clip_image_proj).  The defaults
    are openai/clip-vit-large-patch14: 303,179,776 parameters, 303,966,208 with projection_dim=768.  ``heads`` does not
    shape any tensor; it is listed because the configuration needs it."""
    if hidden % heads or image % patch:
        raise ValueError("hidden must be a multiple of heads and image a multiple of patch")
    sd = OrderedDict()
    sd["embeddings.class_embedding"] = (hidden,)
    sd["embeddings.patch_embedding.weight"] = (hidden, 3, patch, patch)
    sd["embeddings.position_embedding.weight"] = ((image // patch) ** 2 + 1, hidden)

    def norm(name):
        sd[name + ".weight"] = (hidden,)
        sd[name + ".bias"] = (hidden,)

    def linear(name, co, ci):
        sd[name + ".weight"] = (co, ci)
        sd[name + ".bias"] = (co,)

    norm("pre_layrnorm")                                   # (sic: the key of the transformers module)
    for i in range(layers):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            linear(p + "self_attn." + n, hidden, hidden)
        norm(p + "layer_norm1")
        linear(p + "mlp.fc1", intermediate, hidden)
        linear(p + "mlp.fc2", hidden, intermediate)
        norm(p + "layer_norm2")
    norm("post_layernorm")
    if projection_dim:
        sd["visual_projection.weight"] = (projection_dim, hidden)
    return sd


def clip_vision_norm_keys(schema):
    """The LayerNorm tensors of a clip_vision_schema (``norm_keys`` of generate(): their names do not start with 'norm')."""
    return tuple(k for k in schema if k.split(".")[-2] in ("layer_norm1", "layer_norm2", "pre_layrnorm", "post_layernorm"))


def clip_text_schema(vocab=49408, hidden=768, intermediate=3072, layers=12, heads=12, positions=77):
    """Ordered key -> shape of transformers' CLIPTextModel.state_dict() without the ``text_model.`` prefix (SD-1.x's
    text_encoder, the conditioning model of image_descriptors none, ldmseg/models/descriptors.py:98-103).  The defaults are
    openai/clip-vit-large-patch14's text tower: 123,060,480 parameters in 196 tensors.  ``heads`` does not shape any tensor;
    it is listed because the configuration needs it."""
    if hidden % heads:
        raise ValueError("hidden must be a multiple of heads")
    sd = OrderedDict()
    sd["embeddings.token_embedding.weight"] = (vocab, hidden)
    sd["embeddings.position_embedding.weight"] = (positions, hidden)

    def norm(name):
        sd[name + ".weight"] = (hidden,)
        sd[name + ".bias"] = (hidden,)

    def linear(name, co, ci):
        sd[name + ".weight"] = (co, ci)
        sd[name + ".bias"] = (co,)

    for i in range(layers):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            linear(p + "self_attn." + n, hidden, hidden)
        norm(p + "layer_norm1")
        linear(p + "mlp.fc1", intermediate, hidden)
        linear(p + "mlp.fc2", hidden, intermediate)
        norm(p + "layer_norm2")
    norm("final_layer_norm")
    return sd


def clip_text_norm_keys(schema):
    """The LayerNorm tensors of a clip_text_schema (``norm_keys`` of generate())."""
    return tuple(k for k in schema if k.split(".")[-2] in ("layer_norm1", "layer_norm2", "final_layer_norm"))


CLIP_EMBED_KEYS = ("embeddings.class_embedding", "embeddings.position_embedding.weight", "embeddings.token_embedding.weight")
CLIP_EMBED_STD = 0.02       # CLIP initialises the class token, the position table and the token table at this scale


def count_params(schema):
    n = 0
    for shp in schema.values():
        k = 1
        for s in shp:
            k *= s
        n += k
    return n


def _is_norm(key):
    parts = key.split(".")
    leaf = parts[-2]
    return leaf.startswith("norm") or leaf == "conv_norm_out"


def generate(schema, seed=0, device="cpu", dtype=torch.float32, norm_keys=()):
    """Draw a deterministic state dict for ``schema`` (see module docstring)."""
    out = OrderedDict()
    for key, shp in schema.items():
        g = torch.Generator(device="cpu").manual_seed((zlib.crc32(key.encode()) ^ seed) & 0x7FFFFFFF)
        is_norm = _is_norm(key) or key in norm_keys
        u = torch.rand(shp, generator=g, dtype=torch.float32) * 2 - 1
        if key in CLIP_EMBED_KEYS:
            t = CLIP_EMBED_STD * (3.0 ** 0.5) * u             # uniform with standard deviation 0.02
        elif len(shp) == 1:
            if is_norm and key.endswith("weight"):
                t = 1.0 + 0.1 * u
            elif is_norm:
                t = 0.1 * u
            else:
                t = 0.05 * u
        else:
            if len(shp) == 4 and key.startswith("decoder.") and shp[2] == 2:
                fan_in = shp[0]               # ConvTranspose2d k2s2: one tap per output pixel
            else:
                fan_in = 1
                for s in shp[1:]:
                    fan_in *= s
            t = u * (3.0 / fan_in) ** 0.5
        out[key] = t.to(device=device, dtype=dtype)
    return out


VAE_NORM_KEYS = ("encoder.13.weight", "encoder.13.bias", "decoder.3.weight", "decoder.3.bias",
                 "decoder.6.weight", "decoder.6.bias", "decoder.8.weight", "decoder.8.bias")
