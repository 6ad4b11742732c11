#!/usr/bin/env python3
"""Registers, spills and the waves per SIMD they allow, for every kernel of the built library objects.

    tools/kernel_occupancy.py            print the table
    tools/kernel_occupancy.py --write    rewrite tests/golden/kernel_occupancy.json (and kernel_occupancy_msaa.json,
                                         kernel_occupancy_vcolor.json, kernel_occupancy_wino.json,
                                         kernel_occupancy_wino4.json, kernel_occupancy_wino4w.json,
                                         kernel_occupancy_report.json,
                                         kernel_occupancy_view.json, kernel_occupancy_rays.json,
                                         kernel_occupancy_png.json, kernel_occupancy_points.json,
                                         kernel_occupancy_sheet.json, kernel_occupancy_heat.json,
                                         kernel_occupancy_normals.json, kernel_occupancy_backproject.json,
                                         kernel_occupancy_cloudmesh.json, kernel_occupancy_geodesic.json) from the build

A convolution tile's rate depends on how many workgroups a CU holds, i.e. on which side of 168 / 128 / 102 ... registers the
compiler lands - and every epilogue kind compiled into a tile moves that number (round 4: two new kinds took the 80-row tile
from 166 to 191 registers, three resident workgroups per CU to two, conv6 / conv10 of a 12-view pass from 541 to 713 us;
no test saw it, the evidence pass did).  tests/test_host_logic.py::test_kernel_occupancy_table compares the build with the
committed table: fewer waves per SIMD or more spilled registers than recorded fail, on the CPU, at build time.  The multisampled
rasteriser's kernels are built into an object directory of their own (build/msaa/) with a table of their own,
tests/golden/kernel_occupancy_msaa.json, held to the same rule by tests/test_msaa_occupancy.py; so are the tile kernels that
shade with per-vertex colours (build/vcolor/, kernel_occupancy_vcolor.json, tests/test_vcolor_occupancy.py) and the Winograd convolution
tiles (build/wino/, tests/golden/kernel_occupancy_wino.json, tests/test_winograd_occupancy.py), the F(4,3) Winograd tile
(build/wino4/, tests/golden/kernel_occupancy_wino4.json, tests/test_winograd4_occupancy.py), its wide workgroup shape
(build/wino4w/, tests/golden/kernel_occupancy_wino4w.json, tests/test_winograd4_wide_occupancy.py) and the two kernels of the opt-in
landmark report (build/report/, tests/golden/kernel_occupancy_report.json, tests/test_report_occupancy.py) and the six kernels
of the landmark view (build/view/, tests/golden/kernel_occupancy_view.json, tests/test_view_occupancy.py), whose table also
records the bytes of scratch memory per work-item (0); likewise the two kernels of the ray view (build/rays/,
tests/golden/kernel_occupancy_rays.json, tests/test_rays_occupancy.py) and the four kernels of the PNG encoder (build/png/,
tests/golden/kernel_occupancy_png.json, tests/test_png_occupancy.py) and the point-cloud kernels - splat renderer and
nearest-point snap - (build/points/, tests/golden/kernel_occupancy_points.json, tests/test_points_occupancy.py) and the three
kernels of the view sheet (build/sheet/, tests/golden/kernel_occupancy_sheet.json, tests/test_sheet_occupancy.py) and the two
kernels of the heat sheet (build/heat/, tests/golden/kernel_occupancy_heat.json, tests/test_heat_occupancy.py) and the kernels of a
cloud's normals - the estimate and the tile stage that shades with them - (build/normals/,
tests/golden/kernel_occupancy_normals.json, tests/test_normals_occupancy.py) and the three kernels of the surface heat
(build/backproject/, tests/golden/kernel_occupancy_backproject.json, tests/test_backproject_occupancy.py) and the kernels of a
cloud's triangulation (build/cloudmesh/, tests/golden/kernel_occupancy_cloudmesh.json, tests/test_cloudmesh_occupancy.py) and the
kernels of the surface distances between landmarks (build/geodesic/, tests/golden/kernel_occupancy_geodesic.json,
tests/test_geodesic_occupancy.py)."""
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/lib/llvm/bin")
TABLE = REPO / "tests" / "golden" / "kernel_occupancy.json"
MSAA_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_msaa.json"
VCOLOR_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_vcolor.json"
WINO_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_wino.json"
WINO4_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_wino4.json"
WINO4W_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_wino4w.json"
REPORT_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_report.json"
VIEW_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_view.json"
RAYS_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_rays.json"
PNG_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_png.json"
POINTS_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_points.json"
SHEET_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_sheet.json"
HEAT_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_heat.json"
NORMALS_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_normals.json"
BACKPROJECT_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_backproject.json"
CLOUDMESH_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_cloudmesh.json"
GEODESIC_TABLE = REPO / "tests" / "golden" / "kernel_occupancy_geodesic.json"
BUILD = REPO / "mvlm_amd" / "csrc" / "build"


def waves_per_simd(vgprs: int) -> int:
    """gfx950: 512 vector registers per SIMD lane, allocated in blocks of 8, at most 8 waves."""
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def object_kernels(obj: Path) -> dict:
    with tempfile.TemporaryDirectory() as td:
        fat = Path(td) / "fat.bin"
        subprocess.run([str(LLVM / "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", str(obj), str(fat)], check=True)
        data = fat.read_bytes()
        out, i, n = {}, 0, 0
        while True:
            j = data.find(b"\x7fELF", i)
            if j < 0:
                break
            k = data.find(b"\x7fELF", j + 4)
            elf = Path(td) / f"co{n}.elf"
            elf.write_bytes(data[j:k if k > 0 else len(data)])
            notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(elf)], capture_output=True, text=True).stdout
            for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
                nm = re.search(r"\.name:\s+(\S+)", blk)
                vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
                sp = re.search(r"\.vgpr_spill_count:\s+(\d+)", blk)
                sc = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if nm and vg and sp:
                    out[nm.group(1)] = {"vgprs": int(vg.group(1)), "spilled": int(sp.group(1)),
                                                       "waves_per_simd": waves_per_simd(int(vg.group(1))),
                                                       "scratch": int(sc.group(1)) if sc else 0}
            n += 1
            i = j + 4
    return out


def build_table(objdir: Path = BUILD) -> dict:
    table = {}
    for obj in sorted(objdir.glob("*.o")):
        table.update(object_kernels(obj))
    return dict(sorted(table.items()))


if __name__ == "__main__":
    for table_path, objdir in ((TABLE, BUILD), (MSAA_TABLE, BUILD / "msaa"), (VCOLOR_TABLE, BUILD / "vcolor"),
                                (WINO_TABLE, BUILD / "wino"), (WINO4_TABLE, BUILD / "wino4"), (WINO4W_TABLE, BUILD / "wino4w"), (REPORT_TABLE, BUILD / "report"),
                                (VIEW_TABLE, BUILD / "view"), (RAYS_TABLE, BUILD / "rays"), (PNG_TABLE, BUILD / "png"),
                                (POINTS_TABLE, BUILD / "points"), (SHEET_TABLE, BUILD / "sheet"), (HEAT_TABLE, BUILD / "heat"),
                                (NORMALS_TABLE, BUILD / "normals"), (BACKPROJECT_TABLE, BUILD / "backproject"),
                                (CLOUDMESH_TABLE, BUILD / "cloudmesh"), (GEODESIC_TABLE, BUILD / "geodesic")):
        t = build_table(objdir)
        if "--write" in sys.argv:
            fields = ("waves_per_simd", "spilled", "scratch") if table_path in (VIEW_TABLE, RAYS_TABLE, PNG_TABLE, POINTS_TABLE, SHEET_TABLE, HEAT_TABLE, NORMALS_TABLE, BACKPROJECT_TABLE, CLOUDMESH_TABLE, GEODESIC_TABLE) else ("waves_per_simd", "spilled")
            table_path.write_text(json.dumps({k: {f: v[f] for f in fields} for k, v in t.items()}, indent=1) + "\n")
            print(f"{len(t)} kernels -> {table_path}")
        else:
            for k, v in t.items():
                print(f"{v['vgprs']:4d} regs  {v['waves_per_simd']} waves/SIMD  {v['spilled']:3d} spilled  {k}")
