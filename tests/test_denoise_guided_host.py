"""CPU tests of variance-guided denoised frames (include/rays1.h): every new name is declared, exported and bound;
r1_denoise_guided_host equals the contract restated in numpy (tests/guided_cases.py) bit for bit on rendered and synthetic frames whose
variance frames hold every class of value the contract names, under option sets that cover both flag values and both ends of every range;
pixels without a hit keep L's bits and no NaN of theirs reaches an output; out == L; strides with sentinel bytes; every refusal of the check;
the quality test on the medium scene; the census of the new kernels; and, against float64 (tests/filter_truth_cases.py), the
restatement and the host form within a derived rounding bound of the contract's prose, and the cases shown to tell each named mistake of
the guided filter apart.  What the device computes: tests/test_gpu_denoise_guided.py.  Only the quality test and the float64 tests have a
bound."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

import denoise_cases as dc
import filter_truth_cases as tc
import guided_cases as gc
import linear_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("r1_denoise_guided_check", "r1_denoise_guided_host", "r1_denoise_guided_device", "r1_denoise_guided", "r1_render_denoised_guided",
       "r1_render_denoised_guided_device")
CASES = list(dc.RENDERED) + list(dc.SYNTHETIC)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_every_new_name_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rays1.h")).read(), flags=re.S)
    names = {s[0] for s in binding.SYMBOLS}
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(r1.lib(), name) and name in names, name
    assert re.search(r"#define R1_ABI_VERSION 4\b", hdr)
    assert C.sizeof(binding.DenoiseGuidedOpt) == 28 and C.sizeof(binding.DenoiseGuidedFrame) == 24 and C.sizeof(binding.DenoiseOpt) == 20
    for m in ("denoise_guided", "denoise_guided_device", "render_denoised_guided", "render_denoised_guided_device"):
        assert callable(getattr(binding.Renderer, m, None)), m
    for fn in ("make_denoise_guided_opt", "denoise_guided_host", "denoise_guided_check"):
        assert callable(getattr(binding, fn, None)), fn


@pytest.mark.parametrize("options", sorted(gc.OPTION_SETS))
@pytest.mark.parametrize("name", CASES)
def test_host_form_equals_the_numpy_form(name, options):
    L, f, V, it = gc.inputs(name)
    kw = dict(gc.OPTION_SETS[options])
    kw.setdefault("iterations", it)
    o = gc.opt(**kw)
    want = gc.numpy_guided(L, f, V, o)
    got = binding.denoise_guided_host(L, f, V, o)
    assert got.shape == want.shape and int((bits(got) != bits(want)).sum()) == 0, (name, options)
    none = f["hits"] == 0
    assert bits(got)[none].tobytes() == bits(L)[none].tobytes()  # pixels without a hit keep L's bits


@pytest.mark.parametrize("name", ["37x21", "70x40"])
def test_synthetic_variance_frames_hold_every_class_of_input(name):
    L, f, V, _ = gc.inputs(name)
    k = gc.v_classes(f, V)
    for what in ("2x2 blocks of var 0 on hit pixels", "values of 1e30 on hit pixels", "subnormal values on hit pixels", "NaN on pixels without a hit",
                 "hit pixels alone in their 3x3"):
        assert k[what] > 0, (what, k)
    assert k["NaN on hit pixels"] == 0
    # the NaN of the pixels without a hit reaches no output: an output that is NaN is so without them too
    out = gc.host_result(name)
    V0 = V.copy()
    V0["var"][f["hits"] == 0] = 0
    assert bits(binding.denoise_guided_host(L, f, V0, gc.opt(iterations=gc.inputs(name)[3]))).tobytes() == bits(out).tobytes()


# ---- against the float64 truth ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("flags", tc.FLAGS)
@pytest.mark.parametrize("name", list(tc.CASES))
def test_restatement_and_host_form_are_the_float64_truth_within_the_bound(name, flags):
    """max |out - truth| <= (32 + 2^k / 4) n u max |truth|, and pixels without a hit carry L's bits (their variance is NaN: never read)"""
    L, f, V = tc.inputs(name)
    o = tc.options(name, flags, guided=True)
    a = tc.check_against_truth(gc.numpy_guided(L, f, V, o), name, flags, True, "numpy_denoise_guided")
    b = tc.check_against_truth(binding.denoise_guided_host(L, f, V, o), name, flags, True, "r1_denoise_guided_host")
    assert a == b  # (the two are one frame bit for bit)


@pytest.mark.parametrize("mistake", tc.GUIDED_MISTAKES + tc.SHARED_MISTAKES)
def test_the_truth_cases_tell_the_mistakes_apart(mistake):
    """float64 only: each named mistake, made in truth_filter, moves the guided truth of some case by at least 100 times that case's bound"""
    ratios = {}
    for name in ("general 41x23", "general 7x5"):
        o = tc.options(name, 0, True).base
        for flags in tc.FLAGS:
            ratios[name, flags] = tc.shift_in_units(name, flags, True, mistake) / tc.bound_in_units(o.iterations, o.normal_power_log2)
    print(mistake, {k: f"{v:.3g}" for k, v in ratios.items()})
    assert max(ratios.values()) >= 100, (mistake, ratios)
    if mistake == "v over a, not a^2":  # a mistake of demodulation alone
        assert ratios["general 41x23", 0] == 0 and ratios["general 41x23", binding.DENOISE_DEMODULATE] >= 100


@pytest.mark.parametrize("name", ["medium", "37x21"])
def test_out_aliased_to_L_equals_the_result_without_aliasing(name):
    L, f, V, it = gc.inputs(name)
    work = np.array(L)
    got = binding.denoise_guided_host(work, f, V, gc.opt(iterations=it), out=work)
    assert got is work and bits(work).tobytes() == bits(gc.host_result(name)).tobytes()


@pytest.mark.parametrize("name", ["medium", "37x21"])
def test_strides_with_sentinel_bytes_between_the_rows_stay_untouched(name):
    L, f, V, it = gc.inputs(name)
    h, w = L.shape[:2]
    Lv, Lb = dc.strided(L, w + 3)
    fv, fb = dc.strided(f, w + 1)
    Vv, Vb = dc.strided(V, w + 2)
    ov, ob = dc.strided(np.zeros_like(L), w + 5)
    before = [Lb.tobytes(), fb.tobytes(), Vb.tobytes()]
    got = binding.denoise_guided_host(Lv, fv, Vv, gc.opt(iterations=it), out=ov)
    assert bits(got).tobytes() == bits(gc.host_result(name)).tobytes()
    assert [Lb.tobytes(), fb.tobytes(), Vb.tobytes()] == before
    assert (ob[:, w:].view(np.uint8) == dc.PREFILL).all()


def test_every_refusal_of_the_check_with_its_text():
    Lb = r1.lib()
    good_f = binding.DenoiseGuidedFrame(8, 4, 0, 0, 0, 0)
    assert binding.denoise_guided_check(good_f, gc.opt())
    assert binding.denoise_guided_check(binding.DenoiseGuidedFrame(8, 4, 8, 9, 10, 11), gc.opt())
    bad = [(binding.DenoiseGuidedFrame(0, 4, 0, 0, 0, 0), gc.opt(), "width"), (binding.DenoiseGuidedFrame(8, 0, 0, 0, 0, 0), gc.opt(), "height"),
           (binding.DenoiseGuidedFrame(8, 4, 7, 0, 0, 0), gc.opt(), "linear_stride"), (binding.DenoiseGuidedFrame(8, 4, 0, 7, 0, 0), gc.opt(), "feature_stride"),
           (binding.DenoiseGuidedFrame(8, 4, 0, 0, 7, 0), gc.opt(), "moment_stride"), (binding.DenoiseGuidedFrame(8, 4, 0, 0, 0, 7), gc.opt(), "out_stride"),
           (good_f, gc.opt(iterations=0), "iterations"), (good_f, gc.opt(iterations=9), "iterations"), (good_f, gc.opt(normal_power_log2=11), "normal_power_log2"),
           (good_f, gc.opt(sigma_color=0.0), "sigma_color"), (good_f, gc.opt(sigma_depth=float("nan")), "sigma_depth"), (good_f, gc.opt(flags=2), "flags"),
           (good_f, gc.opt(variance_floor=0.0), "variance_floor"), (good_f, gc.opt(variance_floor=-1.0), "variance_floor"),
           (good_f, gc.opt(variance_floor=float("inf")), "variance_floor"), (good_f, gc.opt(variance_floor=float("nan")), "variance_floor"),
           (good_f, gc.opt(reserved=1), "reserved")]
    for fr, o, field in bad:
        with pytest.raises(binding.R1Error) as e:
            binding.denoise_guided_check(fr, o)
        assert e.value.code == binding.R1_EINVAL and field in str(e.value), (field, e.value)
    with pytest.raises(binding.R1Error) as e:
        binding.denoise_guided_check(binding.DenoiseGuidedFrame(65536, 32768, 0, 0, 0, 0), gc.opt())
    assert e.value.code == binding.R1_ELIMIT
    assert Lb.r1_denoise_guided_check(None, C.byref(gc.opt())) == binding.R1_EINVAL and "frame is NULL" in Lb.r1_last_error().decode()
    assert Lb.r1_denoise_guided_check(C.byref(good_f), None) == binding.R1_EINVAL and "options is NULL" in Lb.r1_last_error().decode()
    # the host form: the check first, then the pointers; nothing is written
    L, f, V, _ = gc.inputs("5x3")
    out = np.full(L.shape, 7, np.float32)
    fr = binding.DenoiseGuidedFrame(5, 3, 0, 0, 0, 0)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for args, text in (((ptr(L), ptr(f), ptr(V), None), "out is NULL"), ((ptr(L), ptr(f), None, ptr(out)), "V is NULL"), ((ptr(L), None, ptr(V), ptr(out)), "f is NULL"),
                       ((None, ptr(f), ptr(V), ptr(out)), "L is NULL")):
        assert Lb.r1_denoise_guided_host(C.byref(fr), C.byref(gc.opt()), *args) == binding.R1_EINVAL and text in Lb.r1_last_error().decode()
    assert Lb.r1_denoise_guided_host(C.byref(fr), C.byref(gc.opt(variance_floor=0.0)), ptr(L), ptr(f), ptr(V), ptr(out)) == binding.R1_EINVAL
    assert (out == 7).all()
    # the device forms refuse a null context first, without a device
    p = r1.make_params(16, 8, 2)
    for call in (lambda: Lb.r1_denoise_guided_device(None, None, None, None, None, None, None, None), lambda: Lb.r1_denoise_guided(None, None, None, None, None, None, None, None),
                 lambda: Lb.r1_render_denoised_guided(None, C.byref(p), None, None, None, None), lambda: Lb.r1_render_denoised_guided_device(None, None, None, None, None, None)):
        assert call() == binding.R1_EINVAL and "ctx is NULL" in Lb.r1_last_error().decode()
    # the unguided check keeps refusing unknown flags
    with pytest.raises(binding.R1Error):
        binding.denoise_check(binding.DenoiseFrame(8, 4, 0, 0, 0), dc.opt(flags=2))


# ---- quality ------------------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def medium_reference():
    sa = lc.scene_arrays("medium", 160, 100)
    ref, _ = binding.render_linear_host(lc.cscene(sa), lc.ccamera(sa), r1.make_params(160, 100, 512, 777))
    return sa, ref


@pytest.mark.parametrize("spp", [16, 4])
def test_the_defaults_beat_the_noisy_frame_and_at_16_spp_the_unguided_filter(medium_reference, spp):
    """medium 160 x 100, three iterations, the chosen defaults, against 512 spp at seed 777: RMSE(guided) <= RMSE(noisy) at 16 and 4 spp and
    RMSE(guided) <= RMSE(unguided with dc.OPT) at 16 spp.  Measured here: 16 spp guided 0.6111 of the noisy error, unguided 0.8948; 4 spp
    guided 0.5326 (unguided 0.5615)."""
    sa, ref = medium_reference
    p = r1.make_params(160, 100, spp, 4242)
    L, V, _ = binding.render_moments_host(lc.cscene(sa), lc.ccamera(sa), p)
    f = binding.render_features_host(lc.cscene(sa), lc.ccamera(sa), p)
    guided = dc.rmse(binding.denoise_guided_host(L, f, V, gc.opt()), ref)
    plain = dc.rmse(binding.denoise_host(L, f, dc.opt()), ref)
    noisy = dc.rmse(L, ref)
    print(f"medium 160x100x{spp}: RMSE noisy {noisy:.5f}, guided / noisy {guided / noisy:.4f}, unguided / noisy {plain / noisy:.4f}")
    assert guided <= noisy
    if spp == 16:
        assert guided <= plain


# ---- the drop-in program --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("args", [["--denoise-guided", "--passes", "2"], ["--denoise-guided", "--adaptive", "24"], ["--denoise-guided", "--devices", "2"],
                                  ["--denoise-guided", "0"], ["--denoise-guided", "9"], ["--denoise-guided", "--backend", "cpu-step12"],
                                  ["--denoise-guided", "3", "--gather", "rccl"], ["--variant", "2", "--denoise-guided"], ["--denoise-guided", "--denoise"],
                                  ["--denoise", "2", "--denoise-guided", "2"], ["--denoise-guided", "--spp", "1"], ["--denoise-guided", "--region", "0,0,8,8"]],
                         ids=lambda a: "_".join(a).replace("--", ""))
def test_program_refuses_denoise_guided_with_what_it_cannot_serve_before_touching_a_device(tmp_path, args):
    import subprocess
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    base = ["--width", "32", "--height", "16"] + ([] if "--spp" in args else ["--spp", "8"])
    out = subprocess.run([exe, *base, *args], cwd=tmp_path, capture_output=True, timeout=120)
    assert out.returncode == 1, (out.returncode, out.stderr)
    assert b"--denoise-guided" in out.stderr
    assert b"cannot create HIP context" not in out.stderr
    assert not any(tmp_path.iterdir())  # (nothing rendered, nothing written)


# ---- the built library ------------------------------------------------------------------------------------------------------------------------


def test_census_of_the_guided_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    lib = os.path.join(ROOT, "rays1bench_amd", "lib", "librays1.so")
    if not (os.path.exists(lib) and os.path.exists(kernel_meta.LLVM + "/llvm-objdump")):
        pytest.skip("no library / no LLVM tools")
    k = kernel_meta.collect(lib)
    own = sorted(n for n in k if "r1_vfilter" in n)
    assert sum("r1_vfilter_pass_kernel" in n for n in own) == 4 and sum("r1_vfilter_prepare_kernel" in n for n in own) == 1 and len(own) == 5, own
    assert not any("r1_denoise" in n for n in own)
    for name in own:
        a = k[name]
        print(name, {x: a[x] for x in ("vgpr", "sgpr", "sgpr_spill", "lane_moves", "insts", "lds")})  # (recorded in DESIGN.md §4.40)
        assert a["v_mfma"] == 0 and a["flat_load"] == 0 and a["flat_store"] == 0, (name, a)
        assert int(a["scratch"]) == 0 and a["scratch_insts"] == 0 and int(a["vgpr_spill"]) == 0 and int(a["sgpr_spill"]) == 0, (name, a)
        assert int(a["vgpr"]) <= 128, (name, a["vgpr"])  # four waves a SIMD fit
        staged = "kernelILb1E" in name or "kernel<true" in name  # (mangled or demangled)
        assert int(a["lds"]) == ((32 + 8) * (8 + 8) * (16 + 16 + 4) if staged else 0), (name, a["lds"])


# ---- the stand-alone program ------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tools/check_denoise_guided_host.cpp built with the two host sources it drives, under the address and undefined-behaviour sanitizers: a
    stand-alone program of its own, no GPU, nothing loaded into another process."""
    import subprocess
    out = str(tmp_path_factory.mktemp("denoise_guided_host") / "check_denoise_guided_host")
    src = [os.path.join(ROOT, "tools", "check_denoise_guided_host.cpp")] + [os.path.join(ROOT, "rays1bench_amd", "csrc", f) for f in
                                                                          ("r1_denoise_host.cpp",)]
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    assert os.path.isdir(inc), "the HIP headers are needed to compile the library's host sources"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-D__HIP_PLATFORM_AMD__", "-I" + inc] + src + ["-o", out])
    return out


def test_stand_alone_program_under_the_sanitizers(check_program):
    import subprocess
    out = subprocess.run([check_program], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    for says in ("every value the contract's under 5 sets of options", "strides 40, 38, 41, 42", "refusals wrote nothing"):
        assert says in out.stdout
