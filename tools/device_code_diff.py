#!/usr/bin/env python3
"""Device code of two builds of the library's objects, side by side.

    tools/device_code_diff.py OBJDIR_A OBJDIR_B      (e.g. <parent worktree>/mvlm_amd/csrc/build mvlm_amd/csrc/build)

One line per object file of the two directories (sub-directories included): identical, or how many of its kernels differ (an
object only one side has counts as differing when it holds a kernel);
one line per kernel whose instruction stream (mnemonics and operands) differs or that only one side has, with instruction
count, MFMA count, VGPRs, SGPRs and scratch bytes of both sides.  What a refactoring that should not change the machine code
is checked with before any GPU time is spent (done by hand for profiles/r09_wino_loop_disasm_diff.txt).  It only diffs."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conv_loop_mix import LLVM, code_objects, kernel_listings  # noqa: E402

_TEXT = re.compile(r"^\s*([a-z][a-z0-9_]+\s.*?)\s*//\s*[0-9A-Fa-f]+:")
_SYM = re.compile(r"^[0-9a-f]+ <(\S+)>:")
_NOTE = {"vgprs": r"\.vgpr_count:\s*(\d+)", "sgprs": r"\.sgpr_count:\s*(\d+)", "scratch": r"\.private_segment_fixed_size:\s*(\d+)"}


def kernel_texts(elf: Path) -> dict:
    """kernel symbol -> its instructions as text, branch targets by offset (addresses left out)"""
    text = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", str(elf)], capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = _SYM.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = _TEXT.match(line)
        if m and cur is not None:
            cur.append(re.sub(r"\s+", " ", m.group(1)))
    return out


def kernel_resources(elf: Path) -> dict:
    """kernel symbol -> registers and scratch from the code object's metadata note"""
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(elf)], capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(m.group(1)) if (m := re.search(p, block)) else -1 for k, p in _NOTE.items()}
    return out


def object_kernels(obj: Path) -> dict:
    """kernel symbol -> {text, insns, mfma, vgprs, sgprs, scratch} over every code object of the file"""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for elf in code_objects(obj, Path(td)):
            res, texts = kernel_resources(elf), kernel_texts(elf)
            for name, insns in kernel_listings(elf).items():
                if name in res:
                    out[name] = dict(res[name], text=texts.get(name, []), insns=len(insns), mfma=sum(mn.startswith(("v_mfma", "v_smfmac")) for _, mn, _ in insns))
    return out


def _counts(k) -> str:
    return "absent" if k is None else f"{k['insns']} insns {k['mfma']} mfma {k['vgprs']} vgprs {k['sgprs']} sgprs {k['scratch']} scratch"


def main(dir_a: Path, dir_b: Path) -> int:
    names = sorted({str(p.relative_to(d)) for d in (dir_a, dir_b) for p in d.rglob("*.o")})
    n_differ = 0
    for n in names:
        pa, pb = dir_a / n, dir_b / n
        if not (pa.is_file() and pb.is_file()):
            only = object_kernels(pa if pa.is_file() else pb)  # (a unit without kernels adds or removes no device code)
            print(f"{n}: only in {dir_a if pa.is_file() else dir_b}, {len(only)} kernels")
            n_differ += bool(only)
            continue
        ka, kb = object_kernels(pa), object_kernels(pb)
        differ = [k for k in sorted(set(ka) | set(kb)) if k not in ka or k not in kb or ka[k]["text"] != kb[k]["text"]
                  or any(ka[k][f] != kb[k][f] for f in ("vgprs", "sgprs", "scratch"))]
        print(f"{n}: {len(set(ka) | set(kb))} kernels, " + ("identical" if not differ else f"{len(differ)} differ"))
        for k in differ:
            print(f"    {k}: {_counts(ka.get(k))} | {_counts(kb.get(k))}")
        n_differ += bool(differ)
    print(f"{len(names)} objects, {n_differ} with differing device code")
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(Path(sys.argv[1]), Path(sys.argv[2])))
