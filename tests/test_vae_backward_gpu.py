"""ldmseg_vae_decode_backward and ldmseg_vae_load_decoder on the GPU: every gradient of the decoder against the fp64
torch-CPU reference of tests/vae_backward_ref.py (metric max|g - g64| / max|g64|, bound 1e-3, "fp32" and "bf16x3"; torch's own fp32
CPU autograd is printed beside it), the structural properties of the entry, and the proof that every kernel it launches is compared
by a per-kernel check."""
import pytest
import torch

import vae_backward_ref as R
import vae_backward_run as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ldmseg_amd import _lib
    return _lib.lib()


def all_keys(name):
    return R.decoder_keys(R.CONFIGS[name])


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.ALL_SHAPES, ids=ident)
def test_all_gradients_vs_fp64_reference(case, mode):
    name, B, L = case
    torch.set_num_threads(16)
    z, gl = R.inputs(name, B, L)
    got = G.decode_backward(G.vae(name, mode), z, gl, all_keys(name))
    r64, r32 = R.reference(name, B, L), R.reference_fp32(name, B, L)
    assert set(got) == set(r64)
    worst = {}
    for k in r64:
        e, e32 = R.metric(got[k], r64[k]), R.metric(r32[k], r64[k])
        print(f"{name} B={B} L={L} {mode} {k}: library {e:.3e}  torch fp32 CPU {e32:.3e}")
        c = R.tensor_class(k)
        worst[c] = max(worst.get(c, 0.0), e)
    print(f"{name} B={B} L={L} {mode} worst per class: " + ", ".join(f"{c} {e:.2e}" for c, e in sorted(worst.items())))
    for k in r64:
        assert torch.isfinite(got[k]).all(), k
        assert R.metric(got[k], r64[k]) < R.BOUND, (case, mode, k)


@pytest.mark.parametrize("mode", R.MODES)
def test_z_scale_is_part_of_the_latent_gradient(mode):
    name, B, L = "reduced", 2, 3
    z, gl = R.inputs(name, B, L)
    got = G.decode_backward(G.vae(name, mode), z, gl, all_keys(name), z_scale=0.5)
    want = R.autograd_grads(name, z, gl, torch.float64, z_scale=0.5)
    for k in want:
        assert R.metric(got[k], want[k]) < R.BOUND, k


@pytest.mark.parametrize("mode", R.MODES)
def test_zero_gradient_in_gives_exact_zeros(mode):
    name, B, L = "seg", 2, 3
    z, gl = R.inputs(name, B, L)
    got = G.decode_backward(G.vae(name, mode), z, torch.zeros_like(gl), all_keys(name))
    for k, g in got.items():
        assert torch.count_nonzero(g) == 0, k


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", [("seg", 3, 5), ("reduced", 2, 3)], ids=ident)
def test_no_halo_crosses_an_image(case, mode):
    """grad_logits non-zero in image 0 only: every op of the decoder is per image, so grad_z of the other images is EXACTLY zero"""
    name, B, L = case
    z, gl = R.inputs(name, B, L)
    gl = gl.clone()
    gl[1:] = 0
    got = G.decode_backward(G.vae(name, mode), z, gl, [])
    assert torch.count_nonzero(got["z"][0]) > 0
    assert torch.count_nonzero(got["z"][1:]) == 0


@pytest.mark.parametrize("mode", R.MODES)
def test_batch_gradient_is_the_sum_of_its_images(mode):
    name, B, L = "seg", 3, 5
    z, gl = R.inputs(name, B, L)
    v = G.vae(name, mode)
    whole = G.decode_backward(v, z, gl, all_keys(name))
    parts = [G.decode_backward(v, z[b:b + 1], gl[b:b + 1], all_keys(name)) for b in range(B)]
    for k in all_keys(name):
        total = sum(p[k].double() for p in parts).cpu()
        assert R.metric(whole[k], total) < R.BOUND, k
    assert R.metric(whole["z"], torch.cat([p["z"] for p in parts]).double().cpu()) < R.BOUND


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", [("seg", 2, 3), R.MULTI_SLICE], ids=ident)
def test_two_calls_give_identical_bits(case, mode):
    name, B, L = case
    z, gl = R.inputs(name, B, L)
    v = G.vae(name, mode)
    a = G.decode_backward(v, z, gl, all_keys(name))
    G.vae(name, mode).decode(G.dev(z))                        # another call on the handle in between: the backward keeps no state
    b = G.decode_backward(v, z, gl, all_keys(name))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_absent_and_null_names_leave_the_rest_unchanged():
    name, B, L = "seg", 2, 3
    z, gl = R.inputs(name, B, L)
    v = G.vae(name, "fp32")
    keys = all_keys(name)
    full = G.decode_backward(v, z, gl, keys)
    some = G.decode_backward(v, z, gl, [keys[0], (keys[1], None), keys[5], keys[-2]], want_z=False)
    assert set(some) == {keys[0], keys[5], keys[-2]}
    for k in some:
        assert torch.equal(some[k], full[k]), k
    only_z = G.decode_backward(v, z, gl, [])
    assert torch.equal(only_z["z"], full["z"])


def test_errors_come_with_a_message_and_launch_nothing():
    name, B, L = "seg", 1, 2
    z, gl = R.inputs(name, B, L)
    keys = all_keys(name)
    v, vb = G.vae(name, "fp32"), G.vae(name, "bf16")
    for call, word in ((lambda: G.decode_backward(vb, z, gl, keys, raw=True), "fp32-storage"),
                       (lambda: G.decode_backward(v, z, gl, ["decoder.1.weight"], raw=True), "not a decoder parameter"),
                       (lambda: G.decode_backward(v, z, gl, ["encoder.0.weight"], raw=True), "not a decoder parameter"),
                       (lambda: G.decode_backward(v, z, gl, [keys[0]], numel_of={keys[0]: 7}, raw=True), "elements")):
        (code, msg), names = G.logged(call)
        assert code == -1 and word in msg, (code, msg)
        assert not names, names


def test_load_decoder_errors(lib):
    import ctypes as C
    v = G.vae("seg", "fp32")
    t = torch.zeros(16, device=G.DEV)
    for key, numel in (("decoder.1.weight", 16), ("decoder.0.bias", 16)):
        names, ptrs, numels = (C.c_char_p * 1)(key.encode()), (C.c_void_p * 1)(t.data_ptr()), (C.c_int64 * 1)(numel)
        assert lib.ldmseg_vae_load_decoder(v._h, 1, names, ptrs, numels, None) == -1
        assert lib.ldmseg_last_error()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.ALL_SHAPES, ids=ident)
def test_every_decode_backward_launch_is_compared_per_kernel(lib, case, mode):
    """The dispatch log of one decode_backward call: every kernel name in it (template arguments included) is also logged by the
    per-kernel checks of this configuration - the backward operators against fp64 autograd and the forward operators the recomputation
    launches (G.CHECK, run here with their assertions)."""
    name, B, L = case
    torch.set_num_threads(16)
    z, gl = R.inputs(name, B, L)
    v = G.vae(name, mode)
    _, used = G.logged(lambda: G.decode_backward(v, z, gl, all_keys(name)))
    assert any(n.startswith("wgrad<" + ("x3" if mode == "bf16x3" else "f32")) for n in used), used
    assert any(n.startswith("igemm<") for n in used) and "ln_silu_bwd<f32,pm>" in used and "gn_silu_bwd_stats<f32>" in used

    def per_kernel():
        for kind, q in G.layers(name, B, L):
            G.CHECK[kind](lib, q, mode, forward=True)
    _, tested = G.logged(per_kernel)
    assert used <= tested, sorted(used - tested)
