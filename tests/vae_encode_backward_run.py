"""GPU-side helpers of the encoder-backward tests: objects per (configuration, mode) and the direct call of
ldmseg_vae_encode_backward."""
import ctypes as C
import functools

import torch

import vae_backward_run as G
import vae_encode_backward_ref as R

DEV, P, dev = G.DEV, G.P, G.dev


@functools.lru_cache(maxsize=None)
def vae(name, mode):
    from ldmseg_amd.models import GeneralVAESeg
    return GeneralVAESeg(R.state_dict(name), device=DEV, compute_dtype=mode, scaling_factor=0.2, **R.CONFIGS[name])


def encode_backward(v, name, x, gm, keys, numel_of=None, raw=False, fill=float("nan")):
    """One ldmseg_vae_encode_backward call -> {key: gradient} on the device (raw: (code, message) instead of a check).
    keys: names to ask for; a (key, None) pair passes a NULL pointer for that key."""
    from ldmseg_amd import _lib
    sd = R.state_dict(name)
    xc, gc = dev(x), dev(gm)
    B, _, H, _ = xc.shape
    names, bufs = [], []
    for k in keys:
        null = isinstance(k, tuple)
        k = k[0] if null else k
        names.append(k)
        bufs.append(None if null else torch.full(sd[k].shape, fill, device=DEV) if k in sd else torch.empty(4, device=DEV))
    n = len(names)
    c_names = (C.c_char_p * max(n, 1))(*[k.encode() for k in names])
    c_ptrs = (C.c_void_p * max(n, 1))(*[None if b is None else b.data_ptr() for b in bufs])
    numels = [(numel_of or {}).get(k, sd[k].numel() if k in sd else 4) for k in names]
    c_numels = (C.c_int64 * max(n, 1))(*numels)
    with torch.cuda.device(DEV):
        code = _lib.lib().ldmseg_vae_encode_backward(v._h, P(xc), R.IN_MUL, R.IN_ADD, B, H, P(gc), n, c_names, c_ptrs, c_numels,
                                                     _lib.stream_ptr(torch.device(DEV)))
    if raw:
        msg = _lib.lib().ldmseg_last_error()
        return code, (msg.decode() if msg else "")
    _lib.check(code, "ldmseg_vae_encode_backward")
    torch.cuda.synchronize()
    return {k: b for k, b in zip(names, bufs) if b is not None}
