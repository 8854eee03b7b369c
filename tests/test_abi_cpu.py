"""No-GPU checks of the C-ABI boundary: the shared library loads, exports every symbol that
include/dvsg_amd.h declares, rejects bad arguments with a status code (never aborts), and its
host-only entry point agrees with the oracle.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvsg_amd.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dvsg_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def test_header_declares_the_survey_export_set():
    syms = declared_symbols()
    for s in ["dvsg_tps_solve_f32", "dvsg_tps_warp_f32", "dvsg_flow_warp_f32", "dvsg_stn_sample_f32",
              "dvsg_grid_projective_f32", "dvsg_grid_affine_f32", "dvsg_grid_elastic_f32", "dvsg_locnet_create",
              "dvsg_locnet_destroy", "dvsg_locnet_forward_f32", "dvsg_stabilize_f32", "dvsg_last_error_string"]:
        assert s in syms


def test_library_exports_every_declared_symbol(lib):
    for s in declared_symbols():
        assert hasattr(lib, s), "libdvsg_amd.so does not export %s" % s
    assert lib.dvsg_abi_version() == 1
    assert lib.dvsg_target_arch() == b"gfx950"


def test_python_binding_covers_every_declared_symbol():
    from coupe.dvsg_amd import _lib
    bound = set(_lib.SIGNATURES) | set(_lib.QUERIES)
    assert set(declared_symbols()) == bound


def stream_entry_points():
    """name -> the comment block in front of its declaration group, for every declared function with a `void *stream`
    parameter; whitespace runs collapsed."""
    text = open(HEADER).read()
    out = {}
    for m in re.finditer(r"\bint\s+(dvsg_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", re.sub(r"/\*.*?\*/", lambda c: " " * len(c.group(0)), text, flags=re.S)):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            comments = re.findall(r"/\*.*?\*/", text[:m.start()], flags=re.S)
            out[m.group(1)] = " ".join(comments[-1].split()) if comments else ""
    return out


def test_every_stream_entry_point_is_held_to_the_stream_contract_or_exempt():
    """tests/test_gpu_streams.py registers every entry point that takes a stream (CASES) or names the header's own phrase that
    documents it as synchronous, host-side or debug-only (EXEMPT).  A new entry point fails here until someone decides which.
    Imported without torch: the registry's builders only run on the GPU."""
    import sys
    had_torch = "torch" in sys.modules
    import test_gpu_streams as streams
    assert had_torch or "torch" not in sys.modules, "tests/test_gpu_streams.py imports torch at module level"
    entries = stream_entry_points()
    assert len(entries) >= 60 and "dvsg_stabilize_f32" in entries and "dvsg_scene_step_f32" in entries
    assert "dvsg_locnet_create" not in entries and "dvsg_debug_set_option" not in entries
    cases, exempt = set(streams.CASES), set(streams.EXEMPT)
    assert not cases & exempt, sorted(cases & exempt)
    missing = sorted(set(entries) - cases - exempt)
    assert not missing, "no stream test and no exemption for %s" % missing
    stale = sorted((cases | exempt) - set(entries))
    assert not stale, "registered, but the header declares no such entry point with a stream: %s" % stale
    assert all(streams.CASES[n] for n in cases)
    for name, reason in streams.EXEMPT.items():     # the reason is the header's phrase, in front of that declaration
        assert " ".join(reason.split()) in entries[name], "%s: the header does not say %r" % (name, reason)
        assert re.search(r"synchronous|host|debug", reason + " " + name, flags=re.I), name


def test_every_view_constructor_has_stream_cases():
    """The four source-size renders are registered in tests/test_gpu_streams.py once per row of its VIEWS table, and every view
    constructor the header declares is named by VIEW_CONSTRUCTORS with the rows built through it: a new view property fails
    here until someone gives it a stream case.  Imported without torch, as above."""
    import sys
    had_torch = "torch" in sys.modules
    import test_gpu_streams as streams
    assert had_torch or "torch" not in sys.modules, "tests/test_gpu_streams.py imports torch at module level"
    declared = sorted(s for s in declared_symbols() if s.startswith("dvsg_locnet_view_create"))
    assert len(declared) >= 6 and "dvsg_locnet_view_create" in declared and "dvsg_locnet_view_create_chroma" in declared
    missing = sorted(set(declared) - set(streams.VIEW_CONSTRUCTORS))
    assert not missing, "no view of tests/test_gpu_streams.py is built through %s" % missing
    stale = sorted(set(streams.VIEW_CONSTRUCTORS) - set(declared))
    assert not stale, "named, but the header declares no such constructor: %s" % stale
    for name, labels in streams.VIEW_CONSTRUCTORS.items():
        assert labels, "%s: no label" % name
        unknown = sorted(set(labels) - set(streams.VIEWS))
        assert not unknown, "%s names labels that VIEWS does not have: %s" % (name, unknown)
    # the mapping is what LocNet.view's chain gives for each row's arguments, and every row is a registered case
    for label in streams.VIEWS:
        named = sorted(n for n, labels in streams.VIEW_CONSTRUCTORS.items() if label in labels)
        assert named == sorted(streams.constructors_of(label)) and named, (label, named, streams.constructors_of(label))
    renders = {"dvsg_tps_render_u8": streams.RGB_VIEWS, "dvsg_tps_render_zoom_u8": streams.RGB_VIEWS,
               "dvsg_tps_render_nv12": streams.SURFACE_VIEWS, "dvsg_tps_render_zoom_nv12": streams.SURFACE_VIEWS}
    assert set(streams.RGB_VIEWS) | set(streams.SURFACE_VIEWS) == set(streams.VIEWS)
    for name, labels in renders.items():
        assert [f.label for f in streams.CASES[name]] == [""] + list(labels), name
    for name in ("dvsg_tps_coefficients_f32", "dvsg_tps_coverage_net_f32"):
        assert [f.label for f in streams.CASES[name]] == ["", "shaped"], name


def test_bad_arguments_return_status_not_abort(lib):
    from coupe.dvsg_amd import DvsgError, _lib
    assert lib.dvsg_tps_solve_f32(None, None, 1, 1, 25, None, None) == -1
    assert b"NULL" in lib.dvsg_last_error_string()
    assert lib.dvsg_tps_solve_f32(8, 8, 1, 1, 99, 8, None) == -1
    assert b"P=99" in lib.dvsg_last_error_string()
    assert lib.dvsg_flow_warp_f32(8, 8, 0, 4, 4, 3, 8, None) == -1
    assert lib.dvsg_scale_rgb_f32(8, 1, 4, 4, 4, 8, None) == -1          # C not a multiple of 3
    assert lib.dvsg_grid_elastic_f32(8, 8, 8, 100, None, 1, 4, 4, 3, 4, 4, None, 8, 8, None) == -1
    assert lib.dvsg_prof_end(None, None, None, None) == -1               # not armed
    with pytest.raises(DvsgError, match="dvsg_locnet_workspace_bytes"):
        _lib.call("dvsg_locnet_workspace_bytes", None, 1, 8, 8, None)


DEBUG_OPTION_DEFAULTS = {
    "conv_variant": 0, "conv1_variant": 0, "wide16_min_tiles": 128, "wide16_packed": 1, "wide16_arows": 1,
    "wide16_hreuse": 1, "fused_hreuse": 1, "fuse_conv": 1, "fuse_shortcut": 1, "concat_sc": 1, "x3_conv1": 1, "x3_fuse": 3,
    "f16_split": 1, "f16_pair_mask": 0xFFFF, "flow_tiled": 1, "flow_rounds": 4, "warp_xcd": 0}


def test_debug_options_are_one_table(lib):
    """dvsg_debug_set_option knows the 17 switches and nothing else, and the header names every one of them.  The setter
    makes no HIP call; only defaults are set, so the process is left as it was found."""
    assert len(DEBUG_OPTION_DEFAULTS) == 17
    for name, default in DEBUG_OPTION_DEFAULTS.items():
        assert lib.dvsg_debug_set_option(name.encode(), default) == 0, name
    assert lib.dvsg_debug_set_option(b"no_such_option", 1) == -1
    assert b"no_such_option" in lib.dvsg_last_error_string()
    assert lib.dvsg_debug_set_option(None, 1) == -1
    text = open(HEADER).read()
    comments = re.findall(r"/\*.*?\*/", text[:text.index("int dvsg_debug_set_option(")], flags=re.S)
    for name in DEBUG_OPTION_DEFAULTS:
        assert '"%s"' % name in comments[-1], "include/dvsg_amd.h does not document %s" % name


def test_locnet_create_rejects_incomplete_checkpoint(lib):
    """Runs before any device work: a missing array is DVSG_ERR_WEIGHTS (-4)."""
    name = (ctypes.c_char_p * 1)(b"stabNet/localizationNet/df/dense1/b:0")
    arr = np.zeros(2048, np.float32)
    data = (ctypes.c_void_p * 1)(arr.ctypes.data)
    nd = (ctypes.c_int * 1)(1)
    dims = (ctypes.c_int64 * 4)(2048, 1, 1, 1)
    handle = ctypes.c_void_p()
    rc = lib.dvsg_locnet_create(1, name, data, nd, dims, ctypes.byref(handle))
    assert rc == -4 and b"conv1/weights" in lib.dvsg_last_error_string()
    assert not handle.value


@pytest.mark.parametrize("g", [4, 3, 5])
def test_elastic_constants_match_oracle(lib, g):
    from oracle.spatial_transformer import ElasticTransformer
    n = g * g
    src = np.empty((2, n), np.float32)
    linv = np.empty((n, n + 3), np.float32)
    assert lib.dvsg_elastic_constants_f32(g, src.ctypes.data, linv.ctypes.data) == 0
    o = ElasticTransformer((8, 8), param_dim=2 * n, param_dim_per_side=g)
    assert np.array_equal(src, o.source_points)
    assert np.abs(linv - o.L_inv).max() < 5e-4     # float64 vs float32 (LAPACK) inverse


def test_no_cpu_fallback_without_device():
    """The product must fail loudly, not compute on the CPU, when no HIP device is visible."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from coupe.dvsg_amd import DvsgError
    from coupe.dvsg_amd.warp_with_optical_flow import tf_warp
    with pytest.raises(DvsgError, match="no CPU fallback"):
        tf_warp(np.zeros((1, 4, 4, 3), np.float32), np.zeros((1, 4, 4, 2), np.float32), 4, 4)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "coupe")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                text = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f


def _build_c_demo(tmpdir):
    """examples/c_abi_demo.c with gcc as C99: the header is C (not only C++) and every entry point the demo uses links."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("gcc / ROCm headers not available")
    exe = os.path.join(str(tmpdir), "c_abi_demo")
    libdir = os.path.join(ROOT, "coupe", "dvsg_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_abi_demo.c"), "-L" + libdir, "-ldvsg_amd",
           "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def test_header_is_c99_and_the_c_demo_links(tmp_path):
    _build_c_demo(tmp_path)


@pytest.mark.gpu
def test_c_demo_runs_the_known_answer_tests(tmp_path):
    import subprocess
    exe = _build_c_demo(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "all checks passed" in out.stdout


def test_roctx_ranges_are_off_by_default_and_load_on_request():
    """DVSG_ROCTX=1 makes every stage / bottleneck unit open a roctx range; the roctx
    library is found with dlopen at run time and the switch is read once per process."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); from coupe.dvsg_amd import _lib; "
            "print(_lib.load().dvsg_markers_enabled())" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "DVSG_ROCTX"}
    off = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
    on = subprocess.run([sys.executable, "-c", code], env=dict(env, DVSG_ROCTX="1"), capture_output=True, text=True, check=True)
    assert off.stdout.strip() == "0" and on.stdout.strip() == "1", (off.stdout, on.stdout, on.stderr)
