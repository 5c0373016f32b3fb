"""Torch-only restatement of transformers' CLIPTextModel forward (SD-1.x's text_encoder, the conditioning model of the
text-conditioned mode) on a prefix-less state dict, as the reference for the library's CLIP text executor.
tests/test_clip_text_cpu.py pins it against transformers itself (where installed) and against outputs transformers
produced (tests/golden/clip_text.npz); GPU tests import nothing but this file.

No padding mask: the reference trainer passes none, so only the causal mask applies and the rows behind the EOS token are
computed like any other.

`rnd`: a rounding hook applied to every GEMM / attention operand and every stored activation; `bf16_round` makes the
forward a simulation of bf16 storage with fp32 accumulation (it leaves the accumulation order out)."""
import torch
import torch.nn.functional as F


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def strip_prefix(sd):
    return {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()}


def forward(sd, input_ids, heads, eps=1e-5, rnd=None, dtype=torch.float32):
    """-> last_hidden_state [R, T, C] (final_layer_norm of every row)."""
    sd = strip_prefix(sd)
    r = (lambda t: t) if rnd is None else rnd
    W = {k: v.to(dtype) for k, v in sd.items() if torch.is_floating_point(v)}
    ids = input_ids.long()
    B, T = ids.shape
    tok, pos = W["embeddings.token_embedding.weight"], W["embeddings.position_embedding.weight"]
    C = tok.shape[1]
    h = r(tok[ids] + pos[:T].unsqueeze(0))
    d = C // heads
    causal = torch.full((T, T), float("-inf"), dtype=dtype).triu(1)
    layers = 1 + max(int(k.split(".")[2]) for k in W if k.startswith("encoder.layers."))
    for i in range(layers):
        p = f"encoder.layers.{i}."
        y = r(F.layer_norm(h, (C,), W[p + "layer_norm1.weight"], W[p + "layer_norm1.bias"], eps))
        q, k, v = (r(F.linear(y, r(W[p + f"self_attn.{n}_proj.weight"]), W[p + f"self_attn.{n}_proj.bias"]))
                   .view(B, T, heads, d).transpose(1, 2) for n in ("q", "k", "v"))
        a = torch.softmax((q @ k.transpose(-1, -2)) * d ** -0.5 + causal, dim=-1)
        a = r(r(a) @ v).transpose(1, 2).reshape(B, T, C)
        h = r(h + F.linear(a, r(W[p + "self_attn.out_proj.weight"]), W[p + "self_attn.out_proj.bias"]))
        y = r(F.layer_norm(h, (C,), W[p + "layer_norm2.weight"], W[p + "layer_norm2.bias"], eps))
        y = F.linear(y, r(W[p + "mlp.fc1.weight"]), W[p + "mlp.fc1.bias"])
        y = r(y * torch.sigmoid(1.702 * y))
        h = r(h + F.linear(y, r(W[p + "mlp.fc2.weight"]), W[p + "mlp.fc2.bias"]))
    return F.layer_norm(h, (C,), W["final_layer_norm.weight"], W["final_layer_norm.bias"], eps)


def prompt_ids(starts, T, vocab, seed=0):
    """[len(starts), T] ids shaped like tokenised prompts: BOS, random tokens, EOS (= vocab - 1, CLIP's padding token too)
    from position starts[r] on."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab - 2, (len(starts), T), generator=g)
    ids[:, 0] = vocab - 2
    for r_, s in enumerate(starts):
        ids[r_, s:] = vocab - 1
    return ids


def rel_err(a, b):
    """max-norm relative error, the suite's parity figure"""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


SMALL = dict(vocab=512, hidden=128, intermediate=512, layers=2, heads=2, positions=77)
FULL = dict(vocab=49408, hidden=768, intermediate=3072, layers=12, heads=12, positions=77)
