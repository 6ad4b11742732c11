#!/usr/bin/env python3
"""Instruction mix of the steady-state K loop of every convolution kernel of the built library objects.

    tools/conv_loop_mix.py            print the table
    tools/conv_loop_mix.py --write    rewrite tests/golden/conv_loop_mix_wino.json, conv_loop_mix_wino4.json and
                                      conv_loop_mix_wino4w.json (the Winograd kernels' rows) from the build
    tools/conv_loop_mix.py --write-gaps    rewrite tests/golden/conv_gap_mix_wino4.json (the F(4,3) kernels' largest MFMA gap)

A convolution tile is compute-bound by construction: what it loses against the matrix peak is time its waves spend issuing
anything but MFMAs inside the K loop (addresses, staging arithmetic, LDS traffic, waits, branches).  The ratio of those to the
MFMAs can be read off the object file, before any GPU time is spent.  The steady-state loop of a kernel is the innermost
backward branch whose body holds MFMAs and a barrier (the loop over K-chunks); where a kernel has several, the one with the most
MFMAs.  Instructions are classed by the prefix of their mnemonic.  tests/test_winograd_loop_mix.py holds the Winograd kernel
to the committed row, tests/test_winograd4_loop_mix.py the F(4,3) kernel (build/wino4/) to its own,
tests/test_winograd4_wide_loop_mix.py that kernel's wide workgroup shape (build/wino4w/) to its own.

A wave issues in order, so an MFMA covers only what stands directly behind it: the `gap` column is the longest run of other
instructions between two consecutive MFMAs of the loop (waits and the barrier count).  tests/test_winograd4_gap_mix.py holds both
F(4,3) shapes to tests/golden/conv_gap_mix_wino4.json."""
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/lib/llvm/bin")
BUILD = REPO / "mvlm_amd" / "csrc" / "build"
WINO_TABLE = REPO / "tests" / "golden" / "conv_loop_mix_wino.json"
WINO4_TABLE = REPO / "tests" / "golden" / "conv_loop_mix_wino4.json"
WINO4W_TABLE = REPO / "tests" / "golden" / "conv_loop_mix_wino4w.json"
WINO4_GAP_TABLE = REPO / "tests" / "golden" / "conv_gap_mix_wino4.json"  # object directory -> kernel -> largest MFMA gap
WINO4_GAP_DIRS = ("wino4", "wino4w")
CLASSES = ("valu", "lds_read", "lds_write", "global_load", "scalar", "wait", "other")
MFMAS_PER_CHUNK_WINO = 48  # a 4-channel group of the 64 x (8 x 32) Winograd tile: 6 k-steps x 2 cout tiles x 4 GEMMs
MFMAS_PER_CHUNK_WINO4 = 36  # a 4-channel group of the 32 x (16 x 32) F(4,3) tile, and of its 64 x (8 x 32) shape: 6 k-steps x 6 GEMMs

_INSN = re.compile(r"^\s*([a-z][a-z0-9_]+)\s.*//\s*([0-9A-Fa-f]+):")
_SYM = re.compile(r"^([0-9a-f]+) <(\S+)>:")


def classify(mn: str) -> str:
    if mn.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if mn.startswith("s_barrier"):
        return "barrier"
    if mn.startswith("s_waitcnt"):
        return "wait"
    if mn.startswith("ds_"):
        return "lds_read" if mn.startswith(("ds_read", "ds_load")) else "lds_write" if mn.startswith(("ds_write", "ds_store")) else "other"
    if mn.startswith(("global_load", "buffer_load", "flat_load")):
        return "global_load"
    if mn.startswith("s_"):
        return "scalar"
    if mn.startswith("v_"):
        return "valu"
    return "other"


def code_objects(obj: Path, td: Path):
    fat = td / "fat.bin"
    subprocess.run([str(LLVM / "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", str(obj), str(fat)], check=True)
    data = fat.read_bytes()
    i = n = 0
    while True:
        j = data.find(b"\x7fELF", i)
        if j < 0:
            return
        k = data.find(b"\x7fELF", j + 4)
        elf = td / f"co{n}.elf"
        elf.write_bytes(data[j:k if k > 0 else len(data)])
        yield elf
        n += 1
        i = j + 4


def kernel_listings(elf: Path) -> dict:
    """kernel symbol -> [(address, mnemonic, branch target or None)]"""
    text = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", str(elf)], capture_output=True, text=True).stdout
    out, cur, base = {}, None, 0
    for line in text.splitlines():
        m = _SYM.match(line)
        if m:
            base, cur = int(m.group(1), 16), out.setdefault(m.group(2), [])
            continue
        m = _INSN.match(line)
        if not m or cur is None:
            continue
        mn, addr = m.group(1), int(m.group(2), 16)
        target = None
        if mn.startswith(("s_cbranch", "s_branch")):
            t = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", line)
            target = base + int(t.group(1), 16) if t else base if re.search(r"<[^+>]+>\s*$", line.split("//")[0]) else None
        cur.append((addr, mn, target))
    return out


def loop_mix(insns) -> dict | None:
    """The steady-state loop: among the backward branches whose body holds MFMAs and a barrier and no other such loop, the
    one with the most MFMAs."""
    addr_index = {a: i for i, (a, _, _) in enumerate(insns)}
    loops = []
    for i, (a, mn, t) in enumerate(insns):
        if t is not None and t <= a and t in addr_index:
            body = insns[addr_index[t]:i + 1]
            kinds = [classify(m) for _, m, _ in body]
            if "mfma" in kinds and "barrier" in kinds:
                loops.append((addr_index[t], i, kinds))
    inner = [l for l in loops if not any(o is not l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]
    if not inner:
        return None
    _, _, kinds = max(inner, key=lambda l: l[2].count("mfma"))
    row = {"mfma": kinds.count("mfma"), "barriers": kinds.count("barrier")}
    row.update({c: kinds.count(c) for c in CLASSES})
    row["non_mfma"] = sum(row[c] for c in CLASSES) + row["barriers"]
    row["non_mfma_per_mfma"] = round(row["non_mfma"] / row["mfma"], 3)
    row["max_gap"] = max(mfma_gaps(kinds))
    return row


def mfma_gaps(kinds) -> list:
    """The non-MFMA instructions (waits and barriers included) between each two consecutive MFMAs of a loop body, the body
    taken as a cycle: the run behind the last MFMA continues with the run in front of the first."""
    at = [i for i, k in enumerate(kinds) if k == "mfma"]
    gaps = [b - a - 1 for a, b in zip(at, at[1:])]
    return gaps + [len(kinds) - 1 - at[-1] + at[0]]


def gap_table(objdir: Path) -> dict:
    """kernel -> the largest MFMA gap of its steady loop (tests/golden/conv_gap_mix_wino4.json)"""
    return {k: v["max_gap"] for k, v in build_table(objdir).items()}


def build_table(objdir: Path = BUILD) -> dict:
    table = {}
    with tempfile.TemporaryDirectory() as td:
        for obj in sorted(objdir.glob("conv_inst_*.o")):
            for elf in code_objects(obj, Path(td)):
                for name, insns in kernel_listings(elf).items():
                    if "conv_mfma_kernel" not in name and "conv_pair_kernel" not in name:
                        continue
                    row = loop_mix(insns)
                    if row:
                        table[name] = row
    return dict(sorted(table.items()))


if __name__ == "__main__":
    if "--write-gaps" in sys.argv:
        rows = {d: gap_table(BUILD / d) for d in WINO4_GAP_DIRS}
        WINO4_GAP_TABLE.write_text(json.dumps(rows, indent=1) + "\n")
        print(f"{sum(len(v) for v in rows.values())} kernels -> {WINO4_GAP_TABLE}")
    elif "--write" in sys.argv:
        for path, objdir in ((WINO_TABLE, BUILD / "wino"), (WINO4_TABLE, BUILD / "wino4"), (WINO4W_TABLE, BUILD / "wino4w")):
            rows = {k: {c: n for c, n in v.items() if c != "max_gap"} for k, v in build_table(objdir).items()}
            path.write_text(json.dumps(rows, indent=1) + "\n")
            print(f"{len(rows)} kernels -> {path}")
    else:
        hdr = f"{'mfma':>5s} {'other':>6s} {'/mfma':>6s} {'barr':>5s} {'gap':>4s} " + " ".join(f"{c:>11s}" for c in CLASSES)
        print(hdr + "  kernel")
        for objdir in (BUILD, BUILD / "wino", BUILD / "wino4", BUILD / "wino4w"):
            for k, v in build_table(objdir).items():
                print(f"{v['mfma']:5d} {v['non_mfma']:6d} {v['non_mfma_per_mfma']:6.2f} {v['barriers']:5d} {v['max_gap']:4d} " +
                      " ".join(f"{v[c]:11d}" for c in CLASSES) + f"  {k}")
