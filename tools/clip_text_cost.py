"""Cost of the CLIP text encoder: ms per encoder call on [R, 77] ids on the library in its three compute modes, against
what a user had to run before the library had the encoder - transformers' CLIPTextModel with the same weights on the
same GPU in the same process (fp32, and converted to bf16 once with .to(torch.bfloat16)).

  python tools/clip_text_cost.py [--R 16 32] [--warmup 3] [--iters 20]

R = 16 / 32: 8 / 16 prompts with their unconditional halves (the sampler makes two calls of B rows each; one call of 2 B
rows is the same work).  Timing: one HIP-event pair per call after `warmup` calls, median of `iters` calls.  Prints one
JSON line per measurement.  A record, not a gate: the encoder runs once per sample() call."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-segmentation_amd"))

DEV = "cuda:0"
CFG = dict(vocab=49408, hidden=768, intermediate=3072, layers=12, heads=12, positions=77)


def median_ms(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def torch_module(sd, half=False):
    """transformers' CLIPTextModel on the GPU with the weights of `sd`; half: parameters converted to bf16 once"""
    import torch
    import transformers as tf
    c = CFG
    cfg = tf.CLIPTextConfig(vocab_size=c["vocab"], hidden_size=c["hidden"], intermediate_size=c["intermediate"],
                            num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                            max_position_embeddings=c["positions"], hidden_act="quick_gelu", projection_dim=c["hidden"],
                            bos_token_id=c["vocab"] - 2, eos_token_id=c["vocab"] - 1, pad_token_id=c["vocab"] - 1)
    m = tf.CLIPTextModel(cfg)
    pref = any(k.startswith("text_model.") for k in m.state_dict())
    m.load_state_dict({("text_model." + k if pref else k): v for k, v in sd.items()}, strict=False)
    m = m.eval().to(DEV)
    return m.to(torch.bfloat16) if half else m


def prompt_ids(R, seed=0):
    """ids shaped like tokenised prompts: BOS, random tokens, EOS padding; the second half of the rows are empty prompts"""
    import torch
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, CFG["vocab"] - 2, (R, 77), generator=g)
    ids[:, 0] = CFG["vocab"] - 2
    for r in range(R):
        ids[r, (1 if r >= R // 2 else 6 + (5 * r) % 60):] = CFG["vocab"] - 1
    return ids


def main():
    import torch
    from ldmseg_amd import weights
    from ldmseg_amd.models import CLIPTextEncoder
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    schema = weights.clip_text_schema(**CFG)
    sd = weights.generate(schema, seed=13, norm_keys=weights.clip_text_norm_keys(schema))
    ids = {R: prompt_ids(R, R).to(DEV) for R in args.R}
    try:
        mods = {"transformers fp32": torch_module(sd), "transformers bf16 module (.to(bfloat16))": torch_module(sd, half=True)}
    except ImportError:
        mods = {}
        print(json.dumps({"what": "encode", "note": "transformers is not installed: no comparator"}), flush=True)
    for name, m in mods.items():
        for R in args.R:
            def call():
                with torch.no_grad():
                    return m(input_ids=ids[R])[0].float()
            ms = median_ms(call, args.warmup, args.iters)
            print(json.dumps({"what": "encode", "impl": name, "R": R, "T": 77, "ms": round(ms, 3)}), flush=True)
    mods.clear()
    for mode in ("bf16", "bf16x3", "fp32"):
        m = CLIPTextEncoder(sd, device=DEV, compute_dtype=mode)
        for R in args.R:
            ms = median_ms(lambda: m(ids[R])[0], args.warmup, args.iters)
            print(json.dumps({"what": "encode", "impl": "ldmseg_hip " + mode, "R": R, "T": 77, "ms": round(ms, 3)}), flush=True)
        del m


if __name__ == "__main__":
    main()
