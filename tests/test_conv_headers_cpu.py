"""The convolution kernel's six headers (mvlm_amd/csrc/conv_kernel.h lists them), checked without a GPU:

- each compiles on its own for gfx950, i.e. includes what it uses;
- conv_cfg.h, the tile geometry, is plain C++: with conv_variants.h it compiles under the host compiler of the *_sanitized.py
  tests, every variant's Cfg<> holds its static_asserts there, and one figure per variant family is what the code states today;
- the Makefile rebuilds only the conv_inst_* objects (and the link) after an edit of a kernel header, those and the dispatcher
  after an edit of the geometry, and never api.o or raster.o."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from conftest import REPO

CSRC = REPO / "mvlm_amd/csrc"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)
HEADERS = ["conv_cfg.h", "conv_loop.h", "conv_wino.h", "conv_wino4.h", "conv_tile.h", "conv_launch.h"]

GEOMETRY_TU = """
#include "conv_cfg.h"
#include "conv_variants.h"
// every variant's geometry is instantiated, so Cfg<>'s own static_asserts hold under this compiler too
#define X(id, name, ...) static_assert(__VA_ARGS__::LDS_BYTES <= 160 * 1024 && __VA_ARGS__::PIX_T > 0, name);
MVLM_CONV_VARIANTS(X)
#undef X
// the direct tiles: the dominant 128 x (8 x 32) tile
static_assert(Cfg<128, 32, 8, 1, 3, 4>::LDS_BYTES == 49792);
// the F(4,3) tile's wide shape: what conv_inst_q1.hip states
using WideCfg = MVLM_CONV_WINO4_WIDE_CFG;
static_assert(WideCfg::WIDE4 && WideCfg::PH == 12 && WideCfg::PLANE == 408 && WideCfg::XT == 1632 && WideCfg::WT == 4608 && WideCfg::STAGE == 6240);
static_assert(WideCfg::LDS_BYTES == 51968 && WideCfg::WJOBS == 272 && WideCfg::X_ITERS == 2 && WideCfg::W_ITERS == 5);
static_assert(WideCfg::MIN_BLOCKS_PER_CU == 2 && 2 * WideCfg::LDS_BYTES <= 160 * 1024, "two workgroups stay resident per CU");
static_assert(WideCfg::EMT == 1 && WideCfg::ENT == 4 && WideCfg::EPIX == 128 && WideCfg::ECOUT == 32, "a wave finishes one row quad of 32 channels");
// the two Winograd configurations: k-steps = (kx, channel pair) of a 4-channel chunk
#define X(id, name, ...) static_assert(__VA_ARGS__::WINO && __VA_ARGS__::KSTEPS == 6, name);
MVLM_CONV_VARIANTS_W0(X)
#undef X
static_assert(MVLM_CONV_WINO4_CFG::WINO4 && MVLM_CONV_WINO4_CFG::KSTEPS == 6);
int main() { return 0; }
"""


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own(header, tmp_path):
    tu = tmp_path / "tu.hip"
    tu.write_text(f'#include "{header}"\n')
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-x", "hip", f"-I{CSRC}", str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_geometry_is_plain_cxx(tmp_path):
    tu = tmp_path / "geometry.cpp"
    tu.write_text(GEOMETRY_TU)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", f"-I{CSRC}", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _rebuilt(tree: Path, *make_args) -> set:
    """the targets `make -n` would write in the tree's csrc"""
    r = subprocess.run(["make", "-n", "HIPCC=hipcc", *make_args], cwd=tree / "mvlm_amd/csrc", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return set(re.findall(r"^hipcc .* -o (\S+)", r.stdout, re.M))


@pytest.fixture(scope="module")
def built_tree(tmp_path_factory):
    """A copy of the Makefile among empty stand-ins for the sources and, newer than they, for everything `make` builds:
    make -n reads time stamps only, so this is a built tree without a compiler."""
    if shutil.which("make") is None:
        pytest.skip("needs make")
    tree = tmp_path_factory.mktemp("conv_headers")
    csrc = tree / "mvlm_amd/csrc"
    csrc.mkdir(parents=True)
    (tree / "include").mkdir()
    shutil.copy(CSRC / "Makefile", csrc / "Makefile")
    sources = [csrc / p.name for p in CSRC.iterdir() if p.suffix in (".hip", ".h", ".cpp")] + [tree / "include/mvlm_hip.h"]
    for p in sources:
        p.touch()
        os.utime(p, (1_000_000_000, 1_000_000_000))
    for target in sorted(_rebuilt(tree)):
        (csrc / target).parent.mkdir(parents=True, exist_ok=True)
        (csrc / target).touch()
        os.utime(csrc / target, (1_000_000_100, 1_000_000_100))
    assert _rebuilt(tree) == set(), "the stand-in tree is up to date"
    return tree


def test_kernel_edit_rebuilds_the_instantiating_units_only(built_tree):
    after_tile = _rebuilt(built_tree, "-W", "conv_tile.h")
    objs = {t for t in after_tile if t.endswith(".o")}
    assert after_tile - objs == {"../lib/libmvlm_hip.so"}
    assert len(objs) == 19 and all(Path(t).name.startswith("conv_inst_") for t in objs), sorted(objs)
    after_cfg = _rebuilt(built_tree, "-W", "conv_cfg.h")
    assert after_cfg == after_tile | {"build/conv_mfma.o"}
    for other in ("build/raster.o", "build/api.o"):
        assert other not in after_tile and other not in after_cfg
