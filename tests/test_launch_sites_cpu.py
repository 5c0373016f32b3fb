"""CPU suite: every kernel launch of the UNet forward path goes through LDMSEG_LAUNCH / LDMSEG_LAUNCH_GEMM (csrc/kernels.h),
which record the kernel's name - template arguments and run-time form included - in the dispatch log.
tests/test_igemm_shapes_gpu.py compares that log of full forwards with what the per-op oracle tests ran, so a launch that
bypasses the macros would be invisible to that proof.  This scan fails on any bare hipLaunchKernelGGL in the forward-path sources
that is not on the allow-list below (create-time packers, layout kernels and the small kernels around the GEMM path)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "latent-diffusion-segmentation_amd", "csrc")

SOURCES = ["igemm.hip", "norm.hip", "attention.hip", "attention3.hip", "attention4.hip", "attention_fp8.hip", "attention_mx.hip",
           "tfuse.hip", "tproj.hip", "tail.hip", "misc.hip"]

# (file, kernel) -> (why the launch stays out of the dispatch log, the tests that pin the kernel instead: "file::test" under tests/)
ALLOWED = {
    ("igemm.hip", "split_planes_kernel"): ("create time: fp32 weights -> hi | lo planes of a bf16x3 handle (launch_split_planes)",
        ["test_ops_gpu.py::test_split_bf16_gemm_vs_fp32_reference"]),
    ("igemm.hip", "pack_up4_kernel"): ("create time: upsampler conv weights -> the four 2x2 phase kernels (launch_pack_up4)",
        ["test_ops_gpu.py::test_upsampler_conv_as_phase_convs"]),
    ("igemm.hip", "chain_weights_kernel"): ("create time: chained ff.net.2 / proj_out matrix (launch_chain_weights)",
        ["test_ops_gpu.py::test_chained_ff_out_vs_oracle"]),
    ("igemm.hip", "vec_add_kernel"): ("create time: conv2 + conv_shortcut bias of the extra-tap launch (launch_vec_add)",
        ["test_ops_gpu.py::test_resnet_tail_extra_tap"]),
    ("igemm.hip", "concat_rows_kernel"): ("create time: conv2 | conv_shortcut weight rows of the extra-tap launch (launch_concat_rows)",
        ["test_ops_gpu.py::test_resnet_tail_extra_tap"]),
    ("tfuse.hip", "tf_pack_stream_kernel"): ("create time: weight stream of the fused feed-forward kernel",
        ["test_ops_gpu.py::test_transformer_ff_fused_vs_torch_and_unfused"]),
    ("tproj.hip", "tp_pack_stream_kernel"): ("create time: weight stream of the fused transformer entry kernel",
        ["test_ops_gpu.py::test_transformer_in_fused_vs_torch_and_unfused"]),
    ("misc.hip", "pack_concat3_kernel"): ("layout: fp32 NCHW inputs -> NHWC compute dtype at the API boundary",
        ["test_ops_gpu.py::test_conv2d"]),
    ("misc.hip", "time_sinus_kernel"): ("time embedding: sinusoidal features of the timestep (fp32, no compute-mode variants)",
        ["test_time_embed_gpu.py::test_sinusoid_vs_float64", "test_time_embed_gpu.py::test_rows_equal_the_composed_operators"]),
    ("misc.hip", "small_linear_kernel"): ("time embedding MLP (fp32, B rows, no compute-mode variants)",
        ["test_time_embed_gpu.py::test_small_linear_vs_float64", "test_time_embed_gpu.py::test_rows_equal_the_composed_operators"]),
    ("misc.hip", "repack_conv_kernel"): ("create time: conv weight repack",
        ["test_ops_gpu.py::test_conv2d"]),
    ("misc.hip", "repack_convt2_kernel"): ("create time: ConvTranspose2d weight repack",
        ["test_ops_gpu.py::test_convt2_and_bilinear"]),
    ("misc.hip", "repack_rows_kernel"): ("create time: Linear weight repack",
        ["test_ops_gpu.py::test_linear"]),
    ("misc.hip", "repack_rows_scaled_kernel"): ("create time: Linear weight repack with a folded column scale (LayerNorm gamma)",
        ["test_ops_gpu.py::test_layernorm_folded_into_linear"]),
    ("misc.hip", "rowsum_kernel"): ("create time: row sums of the folded LayerNorm weights (epilogue constants)",
        ["test_ops_gpu.py::test_layernorm_folded_into_linear"]),
    ("misc.hip", "bit_encode_kernel"): ("data preparation: COCO bitmap encode, not in the UNet forward",
        ["test_path_gpu.py::test_bitcodec_bit_exact_vs_reference_golden"]),
    ("misc.hip", "bit_decode_kernel"): ("data preparation: COCO bitmap decode, not in the UNet forward",
        ["test_path_gpu.py::test_bitcodec_bit_exact_vs_reference_golden"]),
}


def _strip_comments(txt):
    txt = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), txt, flags=re.S)
    return re.sub(r"//[^\n]*", "", txt)


def _kernel_of(args):
    """kernel identifier of the first launch argument: '(gn_one_kernel<T, 2>)' / 'kern' -> 'gn_one_kernel' / 'kern'"""
    m = re.match(r"\s*\(*\s*([A-Za-z_][A-Za-z0-9_:]*)", args)
    return m.group(1) if m else args[:40]


def bare_launches(name, txt):
    out = []
    txt = _strip_comments(txt)
    for m in re.finditer(r"\bhipLaunchKernelGGL\s*\(", txt):
        line = txt.count("\n", 0, m.start()) + 1
        out.append((line, _kernel_of(txt[m.end():])))
    return out


def logged_launches(txt, macro="LDMSEG_LAUNCH"):
    return re.findall(r"\b" + macro + r"\s*\(", _strip_comments(txt))


def scan(sources):
    """{file: text} -> list of 'file:line kernel' bare launches that are not allow-listed, and the allow-list entries unused"""
    bad, used = [], set()
    for name, txt in sources.items():
        for line, kern in bare_launches(name, txt):
            if (name, kern) in ALLOWED:
                used.add((name, kern))
            else:
                bad.append(f"{name}:{line} {kern}")
    return bad, set(k for k in ALLOWED if k[0] in sources) - used


def read_sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in SOURCES}


def test_forward_path_launches_are_logged():
    bad, stale = scan(read_sources())
    assert not bad, ("kernel launches that bypass LDMSEG_LAUNCH / LDMSEG_LAUNCH_GEMM (the dispatch log the coverage proof reads); route them through "
                     f"it or add an allow-list entry with its reason: {bad}")
    assert not stale, f"allow-list entries without a launch: {sorted(stale)}"


def test_every_forward_family_logs():
    src = read_sources()
    # the families the coverage proof compares: a file that lost its logged launches has lost them to bare ones or to a new path
    for f in ("igemm.hip", "norm.hip", "attention.hip", "attention3.hip", "attention4.hip", "attention_fp8.hip", "attention_mx.hip",
              "tfuse.hip", "tproj.hip", "tail.hip"):
        assert logged_launches(src[f]) or logged_launches(src[f], "LDMSEG_LAUNCH_GEMM"), f
    # the GEMM family (log level 1, what igemm_log(True) has always recorded): igemm instantiations and the fused GEMM kernels
    for f in ("igemm.hip", "tfuse.hip", "tproj.hip", "tail.hip"):
        assert logged_launches(src[f], "LDMSEG_LAUNCH_GEMM"), f
    for f in ("norm.hip", "attention.hip", "attention3.hip", "attention4.hip", "attention_fp8.hip", "attention_mx.hip"):
        assert not logged_launches(src[f], "LDMSEG_LAUNCH_GEMM"), f
    hdr = open(os.path.join(CSRC, "kernels.h")).read()
    assert re.search(r"#define LDMSEG_LAUNCH\(NAME, \.\.\.\) LDMSEG_LAUNCH_AT\(2,", hdr)
    assert re.search(r"#define LDMSEG_LAUNCH_GEMM\(NAME, \.\.\.\) LDMSEG_LAUNCH_AT\(1,", hdr)
    assert "igemm_log_note" in hdr and "hipLaunchKernelGGL(__VA_ARGS__)" in hdr


def test_scan_catches_a_bare_launch():
    """the scan itself: a logged launch turned back into a bare one, in one form per family, is reported"""
    src = read_sources()
    for f, old in (("norm.hip", "LDMSEG_LAUNCH(ln_plan_name(pl, DT), "),       # the one launch site of launch_ln_plan
                   ("attention4.hip", "LDMSEG_LAUNCH(launch_name(\"attn4<d40,%d,%d,%d>\", NST, LAZY, NWV), "),
                   ("tfuse.hip", "LDMSEG_LAUNCH_GEMM(\"mlp_fused<bf16,proj=1>\", ")):
        assert src[f].count(old) == 1, (f, old)
        patched = dict(src)
        patched[f] = src[f].replace(old, "hipLaunchKernelGGL(")
        bad, _ = scan(patched)
        assert len(bad) == 1 and bad[0].startswith(f + ":"), bad
    # comments do not count
    patched = dict(src)
    patched["tail.hip"] = src["tail.hip"] + "\n// hipLaunchKernelGGL(foo_kernel, ...)\n/* hipLaunchKernelGGL(bar) */\n"
    assert scan(patched)[0] == []


def test_every_allowed_launch_names_the_tests_that_pin_it():
    """the other half of the allow-list: a kernel the dispatch log does not see is compared with a reference by the tests named
    next to its reason, and each of them exists under that name in that file"""
    here = os.path.dirname(os.path.abspath(__file__))
    for key, (why, pins) in ALLOWED.items():
        assert why and pins, key
        for pin in pins:
            fname, test = pin.split("::")
            assert re.fullmatch(r"test_\w+_gpu\.py", fname), (key, pin)      # a kernel is pinned where it runs
            txt = open(os.path.join(here, fname)).read()
            assert re.search(r"^def " + re.escape(test) + r"\(", txt, flags=re.M), f"{key}: no test {test} in tests/{fname}"
