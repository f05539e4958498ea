"""The C-ABI shared library loads (no GPU needed) and exports every symbol include/pi3slam_hip.h declares."""
import ctypes
import os
import re

from conftest import ROOT


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pi3_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(built_lib):
    syms = _declared_symbols()
    assert len(syms) >= 20
    dll = ctypes.CDLL(built_lib)
    missing = [s for s in syms if not hasattr(dll, s)]
    assert not missing, f"declared in the header but not exported: {missing}"


def test_ctypes_table_matches_header(built_lib):
    from pi3_slam_amd import lib
    declared = set(_declared_symbols()) - {"pi3_last_error", "pi3_abi_version", "pi3_build_flavor", "pi3_device_count",
                                            "pi3_groupnorm_ws_doubles", "pi3_ba_workspace_doubles"}   # non-int returns, bound by hand in lib.py
    assert declared == set(lib.SIGNATURES), (declared ^ set(lib.SIGNATURES))
    # arity of every binding == number of parameters in the header prototype
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, argt in lib.SIGNATURES.items():
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        nparams = len([p for p in m.group(1).split(",") if p.strip()])
        assert nparams == len(argt), (name, nparams, len(argt))


def test_loads_without_gpu_and_reports_version(built_lib):
    from pi3_slam_amd import lib
    dll = lib.load(require_gpu=False)
    assert dll.pi3_abi_version() == 7
    assert dll.pi3_device_count() >= 0
    assert isinstance(dll.pi3_last_error(), bytes)


def test_ba_workspace_size_is_the_closed_form(built_lib):
    """pi3_ba_workspace_doubles(N, K) is the sum of the bundle adjuster's arrays and their pads (csrc/ba.hip: ba_layout),
    restated here term by term: the footprint a caller allocates is behaviour, and the function that reports it is the
    same one that carves the buffer."""
    from pi3_slam_amd import lib
    dll = lib.load(require_gpu=False)
    slices = 32
    for N, K in ((1, 1), (5, 8), (66, 6), (100, 200), (128, 256)):
        n6, nk, nblk = 6 * N, N * K, (N * K + 255) // 256
        want = (16                                  # state
                + 6 * nk + 3 * nk                   # Cblk, gp
                + 3 * nk + 12 * N                   # pts_new, poses_new
                + 21 * N + 6 * N + 6 * N + 6 * N    # Bblk, gc, dcam, Dcam
                + slices * n6 * n6 + slices * n6    # S_part, rhs_part
                + 2 * n6 * n6                       # S, L
                + 18 * nk * N + 144                 # Eblk + the tile kernel's reads past its last track
                + (nk * N + 7) // 8                 # observation flags (bytes)
                + 3 * nblk + 3 * N                  # cost / model partials per block and per camera
                + 64                                # spare
                + nk + 36 * N * N                   # inverse depth: rho_new, cross blocks
                + 6 * nk                            # damped point inverses
                + 18 * nk * N + 256)                # Y = E Cinv + the tile kernel's reads past its last track
        assert dll.pi3_ba_workspace_doubles(N, K) == want, (N, K)


def test_knob_registry_refuses_names_of_development_variants(built_lib):
    """The product library knows four knobs; a development variant's name must be refused, not accepted and ignored."""
    import pytest
    from pi3_slam_amd import lib
    lib.load(require_gpu=False)
    assert lib.build_flavor() == "product"
    for name in ("gemm_4w", "gemm_ilv", "gemm_mfma32", "attn_frame_nw", "gemm_abl", "bogus"):
        with pytest.raises(lib.Pi3HipError, match="not a knob of this build"):
            lib.set_knob(name, 1)
        with pytest.raises(lib.Pi3HipError):
            lib.get_knob(name)
    before = lib.get_knob("gelu_form")
    lib.set_knob("gelu_form", 1)
    assert lib.get_knob("gelu_form") == 1
    lib.restore_knob("gelu_form", before)
    assert lib.get_knob("gelu_form") == before


def test_product_path_fails_loudly_without_gpu(built_lib):
    """No CPU fallback: on a box without a GPU the op layer must raise, not compute."""
    import pytest
    import torch
    from pi3_slam_amd import lib
    if lib.load(require_gpu=False).pi3_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(lib.Pi3HipError):
        lib.load(require_gpu=True)


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under pi3_slam_amd/ may import it."""
    pkg = os.path.join(ROOT, "pi3_slam_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f


def test_generated_attention_loop_is_in_sync_with_its_generator(tmp_path):
    """pi3_slam_amd/csrc/attn64a_loop.inc (the hand-placed main loop of attn_fwd64a_kernel) is committed generator output:
    tools/gen_attn_asm.py must reproduce it byte for byte, so nobody edits one without the other."""
    import subprocess
    import sys
    out = tmp_path / "loop.inc"
    env = dict(os.environ, A64A_OUT=str(out))
    env.pop("A64A_ABL", None)
    env.pop("A64A_OPT", None)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_attn_asm.py")], check=True, env=env, capture_output=True)
    committed = open(os.path.join(ROOT, "pi3_slam_amd", "csrc", "attn64a_loop.inc")).read()
    assert out.read_text() == committed
    # the loop's fixed registers stay clear of the compiler's share (operands live below v150) and inside the file
    assert '#define A64A_V0 150' in committed and '"v255"' in committed and '"v256"' not in committed
    # attn64b_loop.inc (attn_fwd64b_kernel: one wave per SIMD x 128 rows) = `gen_attn_asm2.py 4 <out> product`
    out_b = tmp_path / "loop_b.inc"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_attn_asm2.py"), "4", str(out_b), "product"], check=True,
                   env=env, capture_output=True)
    committed_b = open(os.path.join(ROOT, "pi3_slam_amd", "csrc", "attn64b_loop.inc")).read()
    assert out_b.read_text() == committed_b
    # its fixed registers: v66..v253 and a192..a255 (Q); the twelve "+a" operands (O, row sums: 144 registers) fit below a192
    assert '"v66"' in committed_b and '"v65"' not in committed_b and '"v254"' not in committed_b
    assert '"a192"' in committed_b and '"a191"' not in committed_b and '"a255"' in committed_b


def test_header_compiles_and_links_from_plain_c(built_lib, tmp_path):
    """The boundary is a C ABI: include/pi3slam_hip.h must be valid C99 (no C++-isms, no torch types) and a plain C
    program must link against the library and call it - what a cgo / JNI / N-API binding of the reference would do."""
    import subprocess
    src = tmp_path / "client.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "pi3slam_hip.h"
int main(void) {
  long v = 0;
  if (pi3_abi_version() != 7) return 1;
  if (strcmp(pi3_build_flavor(), "product") != 0) return 2;
  if (pi3_set_knob("no_such_knob", 1) != PI3_ERR_ARG) return 3;
  if (strlen(pi3_last_error()) == 0) return 4;
  if (pi3_set_knob("gelu_form", 1) != PI3_OK || pi3_get_knob("gelu_form", &v) != 1 || v != 1) return 5;
  if (pi3_unset_knob("gelu_form") != PI3_OK || pi3_get_knob("gelu_form", &v) != 0) return 6;
  /* an entry point with NULL operands must come back with an error code, not crash (no GPU needed) */
  if (pi3_gemm(NULL, 0, NULL, 0, 0, 0, 0, 0, NULL, NULL, NULL, 0, NULL, 0, 0, 0, 0, 0, 0, NULL, 0, 1.0f, 0, NULL) >= 0) return 7;
  printf("c client ok\n");
  return 0;
}
''')
    exe = tmp_path / "client"
    libdir = os.path.dirname(built_lib)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-l:" + os.path.basename(built_lib), "-Wl,-rpath," + libdir],
                   check=True, capture_output=True)
    env = dict(os.environ)
    env.pop("PI3_GELU_FORM", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "c client ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
