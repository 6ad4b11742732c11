#!/usr/bin/env python3
"""Kernel variant per layer kind, measured INSIDE the landmark network (runs on the GPU box).

tools/tune_conv.py times one layer at a time on idle data: the launch re-reads its tensors out of the MALL and has the
chip to itself.  In a forward pass a layer's tensors were written by other layers (from 12 views up they come from HBM),
and a grid with a fractional last round pays for it differently - the ranking of the tiles changes (round 4: conv4.conv1
of a 12-view pass ran at 104 TFLOP/s on the tile that wins the single-layer benchmark at 124).  This tool therefore
times every candidate where it will run: for each (ksize, cin_pad, cout_pad, size, kind) of the network's 3x3 layers and
each kernel variant that can serve it (mvlm_conv_variant_serves), the variant is forced for that key only
(mvlm_conv_set_override), the pass runs launch by launch with per-launch HIP events, and the key's launches (+ the pool
kernels, which a pool-capable tile makes unnecessary) are summed.  One sweep of coordinate descent over the keys, largest
first; winners that beat the current choice by more than 2 % stay in place for the keys after them.

usage: python tools/tune_in_network.py [--batches 8,12,...] [--write-header] [--out gpurun_out/conv_net_tune.json]

--winograd: the table of the Winograd tiles (conv_tuned_wino.h) instead.  Per batch, starting from the direct path (mode 0),
every (shape, kind) a Winograd variant can serve is switched to it alone, largest first; the launches that CHANGED against the
pass before it (the layer's own, the pair launch it left, a second-input form it ended) are summed on both sides, and the key
stays switched where the new launches are faster by more than --min-gain.  An entry names the smallest tuned batch from which
the key won at every tuned batch above it.

--winograd4: the table of the F(4,3) Winograd tile (conv_tuned_wino4.h), the same way, but starting from what runs without that
tile: the default Winograd mode (1, the table conv_tuned_wino.h) with the F(4,3) switch at 0.  A key is switched where the tile
beats the F(2,3) tile, the pair launch or the direct tile that serves it otherwise.

--winograd4-wide: no table, a comparison.  Per batch (default 96,12) the default pass is timed with the F(4,3) tile's workgroup
shape switch (mvlm_cnn_set_winograd4_wide) at 0 and at 1, alternating, and every (shape, kind) whose launches on code 2048 the
wide shape takes (mvlm_conv_wino4_wide_serves) is listed with its time per pass under either setting, then the sum of the
convolution kernels of a pass.  A key that the wide shape makes slower by more than --min-gain is marked; --write-header lists
the keys marked at the largest batch in conv_wino4_wide_hold.h, which the dispatcher keeps on the 32 x 16 shape.  A key the
header already holds runs on that shape under either setting here and cannot be marked again, so its row is carried over: to
measure it afresh, take it out of the header and build first.  --f43-mode 2 (default) puts every key the tile serves on it, 1
leaves the pass to the measured table (no launch of the tile below 96 views).

--winograd4-padded: the table of the 80- and 84-row direct tiles' launches that run on the F(4,3) tile over padded weights
(conv_tuned_wino4_pad.h).  At 96 views (or --batches) the default pass is timed with mvlm_cnn_set_winograd4_padded at 0 and at 2,
alternating, --passes times each, the quietest timing per launch; every (shape, kind) whose launches the switch moves to code 2048
is listed with its time per pass under either setting, then the sum of the convolution kernels of a pass.  A key gets a row where
the tile is faster by more than --min-gain in every net that has it; --write-header writes the rows, each held at 96 views.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from collections import defaultdict
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
HEADER = REPO / "mvlm_amd" / "csrc" / "conv_tuned_net.h"
WINO_HEADER = REPO / "mvlm_amd" / "csrc" / "conv_tuned_wino.h"
WINO4_HEADER = REPO / "mvlm_amd" / "csrc" / "conv_tuned_wino4.h"
WIDE_HOLD_HEADER = REPO / "mvlm_amd" / "csrc" / "conv_wino4_wide_hold.h"
WINO4_PAD_HEADER = REPO / "mvlm_amd" / "csrc" / "conv_tuned_wino4_pad.h"
CAP = 1024


def variant_ids(lib):
    """the base ids the library names (mvlm_conv_variant_name), the split-operand kernels' 61 / 62 aside"""
    return [v for v in range(61) if lib.mvlm_conv_variant_name(v).decode() != "?"]


def wino_ids(lib):
    return [v for v in variant_ids(lib) if lib.mvlm_conv_variant_name(v).decode().startswith("conv3x3w_")]


WINO4_CODE = 2048  # MVLM_CONV_VARIANT_WINO4: the F(4,3) tile is not one of the base ids


def wino4_ids(lib):
    return [WINO4_CODE] if lib.mvlm_conv_variant_name(WINO4_CODE).decode().startswith("conv3x3q_") else []


def profile_pass(pred, images, out, passes):
    """-> list of per-pass record lists [(slot, variant, ms, shape6)]"""
    ctx = pred.ctx
    slot, var = (C.c_int32 * CAP)(), (C.c_int32 * CAP)()
    fl, ms = (C.c_double * CAP)(), (C.c_float * CAP)()
    shapes = (C.c_int32 * (6 * CAP))()
    runs = []
    for _ in range(passes):
        pred.predict_device(images, out=out)
        n = ctx.lib.mvlm_cnn_get_profile(ctx.handle, slot, var, fl, ms, CAP)
        m = ctx.lib.mvlm_cnn_get_profile_shapes(ctx.handle, shapes, CAP)
        assert n == m and n > 0
        runs.append([(slot[i], var[i], ms[i] * 1e3, tuple(shapes[6 * i + k] for k in range(6))) for i in range(n)])
    return runs


def key_time(runs, key):
    """mean us per pass of the launches with this (ksize, cin_pad, cout_pad, size, kind) + all pool-kernel launches"""
    tot = []
    for rec in runs:
        tot.append(sum(t for s, v, t, sh in rec if (s >= 0 and sh[:5] == key and not (v & 0x1000)) or s == -1))
    return float(np.min(tot))  # the quietest pass: clocks and neighbours only ever add time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default=ap_default_batches())
    ap.add_argument("--nets", default="dtu3d:geometry+depth,bu3dfe:RGB+depth")
    ap.add_argument("--write-header", action="store_true")
    ap.add_argument("--merge", action="store_true", help="keep the entries of the existing header that this run does not re-measure")
    ap.add_argument("--out", default=str(REPO / "gpurun_out" / "conv_net_tune.json"))
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--min-gain", type=float, default=0.02)
    ap.add_argument("--max-size", type=int, default=256, help="only keys of feature maps up to this size (re-tuning the small levels)")
    ap.add_argument("--winograd", action="store_true", help="tune the Winograd tiles' table (conv_tuned_wino.h) instead")
    ap.add_argument("--winograd4", action="store_true", help="tune the F(4,3) Winograd tile's table (conv_tuned_wino4.h) instead")
    ap.add_argument("--winograd4-wide", action="store_true", help="time every key the F(4,3) tile's wide workgroup shape serves with the switch at 0 and 1")
    ap.add_argument("--winograd4-padded", action="store_true", help="tune the table of the 80- / 84-row layers that run on the F(4,3) tile over padded weights (conv_tuned_wino4_pad.h)")
    ap.add_argument("--f43-mode", type=int, default=2, help="--winograd4-wide: the F(4,3) mode of the compared passes (2 every served key, 1 the table)")
    ap.add_argument("--hold-min-batch", type=int, default=0,
                    help="--winograd4: write no row below this many views, whatever won there (the header says so and why)")
    ap.add_argument("--header-from", default="", help="--winograd / --winograd4: write the header from this earlier --out JSON, without tuning")
    args = ap.parse_args()
    if (args.winograd or args.winograd4) and args.header_from:
        rows = json.loads(Path(args.header_from).read_text())
        return write_wino_header(rows, sorted({r["batch"] for r in rows}), None, args.winograd4, args.hold_min_batch)
    if args.winograd or args.winograd4:
        return tune_winograd(args, four=args.winograd4)
    if args.winograd4_wide:
        return compare_wide(args)
    if args.winograd4_padded:
        return tune_padded(args)

    import torch

    from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor

    rows = []
    seen_keys = set()  # (key, batch) tuned by an earlier net: the second net only adds what the first does not have
    for net in args.nets.split(","):
        name, mode = net.split(":")
        pred = (DTU3DPredictor if name == "dtu3d" else BU3DFEPredictor)(image_mode=mode, weights="synthetic:0", verbose=False)
        ctx, lib = pred.ctx, pred.ctx.lib
        ids = [v for v in variant_ids(lib) if v not in wino_ids(lib)]  # (the Winograd tiles have tables of their own: --winograd, --winograd4)
        nl = pred.get_lm_count()
        for batch in [int(b) for b in args.batches.split(",")]:
            rs = np.random.RandomState(batch)
            images = torch.from_numpy(rs.rand(batch, 256, 256, 4).astype(np.float32)).cuda()
            out = torch.empty((nl, batch, 3), dtype=torch.float32, device="cuda")
            pred.set_execution(graphs=False)
            ctx.check(lib.mvlm_conv_set_override(ctx.handle, 0, 0, 0, 0, 0, -1))
            pred.predict_device(images, out=out)  # first use: launch attributes, workspace
            ctx.check(lib.mvlm_cnn_set_profiling(ctx.handle, 1))
            t0 = time.time()
            base = profile_pass(pred, images, out, args.passes)
            total0 = min(sum(t for _, _, t, _ in rec) for rec in base)
            keys = defaultdict(float)
            current = {}
            for s, v, t, sh in base[0]:
                if s >= 0 and sh[0] == 3 and not (v & 0x1000) and sh[2] % 32 == 0 and sh[3] <= args.max_size:
                    keys[sh[:5]] += t
                    current[sh[:5]] = v
            gained = 0.0
            for key in sorted(keys, key=lambda k: -keys[k]):
                if (key, batch) in seen_keys:
                    continue
                seen_keys.add((key, batch))
                cands = [v for v in ids if lib.mvlm_conv_variant_serves(v, *key)]
                if key[3] <= 8 and batch <= 32:
                    cands += [v + 256 * lg for v in ids for lg in (1, 2) if lib.mvlm_conv_variant_serves(v + 256 * lg, *key)]
                cur = current[key]
                if len(cands) < 2:
                    continue
                res = {}
                for v in cands:
                    ctx.check(lib.mvlm_conv_set_override(ctx.handle, *key, v))
                    try:
                        res[v] = key_time(profile_pass(pred, images, out, args.passes), key)
                    except Exception as e:  # noqa: BLE001 - a variant that cannot run this layer after all
                        print("   ", lib.mvlm_conv_variant_name(v).decode(), "failed:", e, file=sys.stderr)
                if cur not in res:
                    res[cur] = key_time(base, key)
                best = min(res, key=res.get)
                win = best != cur and res[best] < (1.0 - args.min_gain) * res[cur]
                keep = best if win else cur
                ctx.check(lib.mvlm_conv_set_override(ctx.handle, *key, keep))
                if win:
                    gained += res[cur] - res[best]
                rows.append(dict(net=net, batch=batch, key=list(key), current=cur, current_name=lib.mvlm_conv_variant_name(cur).decode(),
                                 current_us=round(res[cur], 1), best=best, best_name=lib.mvlm_conv_variant_name(best).decode(),
                                 best_us=round(res[best], 1), kept=keep, all_us={str(k): round(v, 1) for k, v in res.items()}))
                mark = f"   <-- {lib.mvlm_conv_variant_name(best).decode()} {res[best]:.1f} us" if win else ""
                print(f"{net} B{batch:3d} k{key[0]} {key[1]:3d}->{key[2]:3d} @{key[3]:3d} kind {key[4]}  {lib.mvlm_conv_variant_name(cur).decode():24s} "
                      f"{res[cur]:9.1f} us{mark}", flush=True)
            final = profile_pass(pred, images, out, args.passes)
            total1 = min(sum(t for _, _, t, _ in rec) for rec in final)
            ctx.check(lib.mvlm_cnn_set_profiling(ctx.handle, 0))
            print(f"== {net} batch {batch}: conv kernels of a pass {total0 / 1e3:.3f} ms -> {total1 / 1e3:.3f} ms "
                  f"(sum of per-key gains {gained:.0f} us; {time.time() - t0:.0f} s)", flush=True)
            rows.append(dict(net=net, batch=batch, summary=True, before_us=round(total0, 1), after_us=round(total1, 1)))
            del images, out
        ctx.check(lib.mvlm_conv_set_override(ctx.handle, 0, 0, 0, 0, 0, -1))
        del pred
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rows, indent=0))
    if args.write_header:
        write_header(rows, args.merge)


def min_records(runs):
    """per launch of a pass the quietest of the passes' timings (the launch sequence of a configuration is fixed)"""
    assert all(len(r) == len(runs[0]) for r in runs)
    return [(runs[0][i][0], runs[0][i][1], min(r[i][2] for r in runs), runs[0][i][3]) for i in range(len(runs[0]))]


def changed_us(before, after):
    """sum of the launches of `before` that `after` does not have with the same (slot, variant), and the other way round"""
    from collections import Counter

    cb, ca = Counter((s, v) for s, v, _, _ in before), Counter((s, v) for s, v, _, _ in after)
    common = cb & ca

    def rest(recs):
        left, tot, rows = Counter(common), 0.0, []
        for s, v, t, sh in recs:
            if left[(s, v)] > 0:
                left[(s, v)] -= 1
            else:
                tot += t
                rows.append((s, v, round(t, 1)))
        return tot, rows

    return rest(before), rest(after)


def tune_winograd(args, four=False):
    import torch

    from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor

    rows = []
    batches = sorted((int(b) for b in args.batches.split(",")), reverse=True)
    for net in args.nets.split(","):
        name, mode = net.split(":")
        pred = (DTU3DPredictor if name == "dtu3d" else BU3DFEPredictor)(image_mode=mode, weights="synthetic:0", verbose=False)
        ctx, lib = pred.ctx, pred.ctx.lib
        wids = wino4_ids(lib) if four else wino_ids(lib)
        nl = pred.get_lm_count()

        def everything_mode(on):  # every servable layer on the tiles being tuned / what runs without them
            if four:
                ctx.check(lib.mvlm_cnn_set_winograd(ctx.handle, 1))
                ctx.check(lib.mvlm_cnn_set_winograd4(ctx.handle, 2 if on else 0))
            else:
                ctx.check(lib.mvlm_cnn_set_winograd(ctx.handle, 2 if on else 0))

        everything_mode(False)
        for batch in batches:
            rs = np.random.RandomState(batch)
            images = torch.from_numpy(rs.rand(batch, 256, 256, 4).astype(np.float32)).cuda()
            out = torch.empty((nl, batch, 3), dtype=torch.float32, device="cuda")
            pred.set_execution(graphs=False)
            ctx.check(lib.mvlm_conv_set_override(ctx.handle, 0, 0, 0, 0, 0, -1))
            pred.predict_device(images, out=out)
            ctx.check(lib.mvlm_cnn_set_profiling(ctx.handle, 1))
            state = min_records(profile_pass(pred, images, out, args.passes))
            total0 = sum(t for _, _, t, _ in state)
            keys = defaultdict(float)
            # which (shape, kind) keys exist: one pass with everything servable switched
            everything_mode(True)
            everything = min_records(profile_pass(pred, images, out, 1))
            everything_mode(False)
            for s, v, t, sh in everything:
                if s >= 0 and v in wids:
                    keys[sh[:5]] += t
            for key in sorted(keys, key=lambda k: -keys[k]):
                best = None
                for v in wids:
                    if not lib.mvlm_conv_variant_serves(v, *key):
                        continue
                    ctx.check(lib.mvlm_conv_set_override(ctx.handle, *key, v))
                    cand = min_records(profile_pass(pred, images, out, args.passes))
                    (us0, rows0), (us1, rows1) = changed_us(state, cand)
                    if best is None or us1 < best[2]:
                        best = (v, us0, us1, rows0, rows1, cand)
                    ctx.check(lib.mvlm_conv_set_override(ctx.handle, *key, -1))
                if best is None:
                    continue
                v, us0, us1, rows0, rows1, cand = best
                win = us1 < (1.0 - args.min_gain) * us0
                if win:
                    ctx.check(lib.mvlm_conv_set_override(ctx.handle, *key, v))
                    state = cand
                rows.append(dict(net=net, batch=batch, key=list(key), variant=v, name=lib.mvlm_conv_variant_name(v).decode(),
                                 direct_us=round(us0, 1), winograd_us=round(us1, 1), kept=bool(win), direct=rows0, winograd=rows1))
                print(f"{net} B{batch:3d} {key[1]:3d}->{key[2]:3d} @{key[3]:3d} kind {key[4]}  direct {us0:9.1f} us ({len(rows0)} launches)  "
                      f"{lib.mvlm_conv_variant_name(v).decode()} {us1:9.1f} us ({len(rows1)} launches)  {us0 / us1:5.2f}x{'  <-- kept' if win else ''}", flush=True)
            total1 = sum(t for _, _, t, _ in state)
            ctx.check(lib.mvlm_cnn_set_profiling(ctx.handle, 0))
            print(f"== {net} batch {batch}: conv kernels of a pass {total0 / 1e3:.3f} ms -> {total1 / 1e3:.3f} ms", flush=True)
            rows.append(dict(net=net, batch=batch, summary=True, before_us=round(total0, 1), after_us=round(total1, 1)))
            del images, out
        ctx.check(lib.mvlm_conv_set_override(ctx.handle, 0, 0, 0, 0, 0, -1))
        if four:
            ctx.check(lib.mvlm_cnn_set_winograd4(ctx.handle, 1))
        ctx.check(lib.mvlm_cnn_set_winograd(ctx.handle, 1))
        del pred
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rows, indent=0))
    if args.write_header:
        write_wino_header(rows, batches, Path(args.out).parent, four, args.hold_min_batch)


def compare_wide(args):
    import torch

    from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor

    rows = []
    batches = [96, 12] if args.batches == ap_default_batches() else [int(b) for b in args.batches.split(",")]
    for net in args.nets.split(","):
        name, mode = net.split(":")
        pred = (DTU3DPredictor if name == "dtu3d" else BU3DFEPredictor)(image_mode=mode, weights="synthetic:0", verbose=False)
        ctx, lib = pred.ctx, pred.ctx.lib
        nl = pred.get_lm_count()
        ctx.check(lib.mvlm_cnn_set_winograd(ctx.handle, 1))
        ctx.check(lib.mvlm_cnn_set_winograd4(ctx.handle, args.f43_mode))
        for batch in batches:
            rs = np.random.RandomState(batch)
            images = torch.from_numpy(rs.rand(batch, 256, 256, 4).astype(np.float32)).cuda()
            out = torch.empty((nl, batch, 3), dtype=torch.float32, device="cuda")
            pred.set_execution(graphs=False)
            runs = {0: [], 1: []}
            for on in (0, 1):  # first use of either shape: launch attributes, workspace
                ctx.check(lib.mvlm_cnn_set_winograd4_wide(ctx.handle, on))
                pred.predict_device(images, out=out)
            ctx.check(lib.mvlm_cnn_set_profiling(ctx.handle, 1))
            for _ in range(args.passes):
                for on in (0, 1):
                    ctx.check(lib.mvlm_cnn_set_winograd4_wide(ctx.handle, on))
                    runs[on] += profile_pass(pred, images, out, 1)
            ctx.check(lib.mvlm_cnn_set_profiling(ctx.handle, 0))
            ctx.check(lib.mvlm_cnn_set_winograd4_wide(ctx.handle, 1))
            rec = {on: min_records(runs[on]) for on in (0, 1)}
            assert [(s, v) for s, v, _, _ in rec[0]] == [(s, v) for s, v, _, _ in rec[1]]  # the switch moves no launch to another code
            keys = {on: defaultdict(float) for on in (0, 1)}
            count = defaultdict(int)
            for on in (0, 1):
                for s, v, t, sh in rec[on]:
                    if s >= 0 and v == WINO4_CODE and lib.mvlm_conv_wino4_wide_serves(*sh[:4]):
                        keys[on][sh[:5]] += t
                        count[sh[:5]] += on
            for key in sorted(keys[0], key=lambda k: -keys[0][k]):
                us0, us1 = keys[0][key], keys[1][key]
                slower = us1 > (1.0 + args.min_gain) * us0
                rows.append(dict(net=net, batch=batch, key=list(key), launches=count[key], narrow_us=round(us0, 1), wide_us=round(us1, 1), slower=bool(slower)))
                print(f"{net} B{batch:3d} {key[1]:3d}->{key[2]:3d} @{key[3]:3d} kind {key[4]}  {count[key]:2d} launches  narrow {us0:9.1f} us  wide {us1:9.1f} us  "
                      f"{us0 / us1:5.2f}x{'  <-- slower on the wide shape' if slower else ''}", flush=True)
            tot = {on: sum(t for _, _, t, _ in rec[on]) for on in (0, 1)}
            f43 = {on: sum(t for _, v, t, _ in rec[on] if v == WINO4_CODE) for on in (0, 1)}
            print(f"== {net} batch {batch}, F(4,3) mode {args.f43_mode}: conv kernels of a pass {tot[0] / 1e3:.3f} ms -> {tot[1] / 1e3:.3f} ms with the wide shape "
                  f"(launches on code 2048: {f43[0] / 1e3:.3f} -> {f43[1] / 1e3:.3f} ms; keys served wide: {sum(keys[0].values()) / 1e3:.3f} -> {sum(keys[1].values()) / 1e3:.3f} ms)", flush=True)
            rows.append(dict(net=net, batch=batch, summary=True, before_us=round(tot[0], 1), after_us=round(tot[1], 1)))
            del images, out
        ctx.check(lib.mvlm_cnn_set_winograd4(ctx.handle, 1))
        del pred
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rows, indent=0))
    if args.write_header:
        write_wide_hold_header(rows, max(batches))


def tune_padded(args):
    import torch

    from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor

    rows = []
    batches = [96] if args.batches == ap_default_batches() else [int(b) for b in args.batches.split(",")]
    for net in args.nets.split(","):
        name, mode = net.split(":")
        pred = (DTU3DPredictor if name == "dtu3d" else BU3DFEPredictor)(image_mode=mode, weights="synthetic:0", verbose=False)
        ctx, lib = pred.ctx, pred.ctx.lib
        nl = pred.get_lm_count()
        for batch in batches:
            rs = np.random.RandomState(batch)
            images = torch.from_numpy(rs.rand(batch, 256, 256, 4).astype(np.float32)).cuda()
            out = torch.empty((nl, batch, 3), dtype=torch.float32, device="cuda")
            pred.set_execution(graphs=False)
            runs = {0: [], 2: []}
            for sw in (0, 2):  # first use of either kernel: launch attributes
                ctx.check(lib.mvlm_cnn_set_winograd4_padded(ctx.handle, sw))
                pred.predict_device(images, out=out)
            ctx.check(lib.mvlm_cnn_set_profiling(ctx.handle, 1))
            for _ in range(args.passes):
                for sw in (0, 2):
                    ctx.check(lib.mvlm_cnn_set_winograd4_padded(ctx.handle, sw))
                    runs[sw] += profile_pass(pred, images, out, 1)
            ctx.check(lib.mvlm_cnn_set_profiling(ctx.handle, 0))
            ctx.check(lib.mvlm_cnn_set_winograd4_padded(ctx.handle, 1))
            rec = {sw: min_records(runs[sw]) for sw in (0, 2)}
            assert [(s, sh) for s, _, _, sh in rec[0]] == [(s, sh) for s, _, _, sh in rec[2]]  # the switch moves kernels, not launches
            keys = {sw: defaultdict(float) for sw in (0, 2)}
            count, direct = defaultdict(int), {}
            for (s, v0, t0, sh), (_, v2, t2, _) in zip(rec[0], rec[2]):
                if v0 != v2:
                    assert v2 == WINO4_CODE, (s, v0, v2)
                    keys[0][sh[:5]] += t0
                    keys[2][sh[:5]] += t2
                    count[sh[:5]] += 1
                    direct[sh[:5]] = v0
            for key in sorted(keys[0], key=lambda k: -keys[0][k]):
                us0, us2 = keys[0][key], keys[2][key]
                faster = us2 * (1.0 + args.min_gain) < us0
                rows.append(dict(net=net, batch=batch, key=list(key), launches=count[key], direct_variant=direct[key], direct_us=round(us0, 1),
                                 padded_us=round(us2, 1), faster=bool(faster)))
                print(f"{net} B{batch:3d} {key[1]:3d}->{key[2]:3d} @{key[3]:3d} kind {key[4]}  {count[key]:2d} launches  variant {direct[key]:2d} {us0:9.1f} us  "
                      f"F(4,3) padded {us2:9.1f} us  {us0 / us2:5.2f}x{'  <-- row' if faster else ''}", flush=True)
            tot = {sw: sum(t for _, _, t, _ in rec[sw]) for sw in (0, 2)}
            print(f"== {net} batch {batch}: conv kernels of a pass {tot[0] / 1e3:.3f} ms -> {tot[2] / 1e3:.3f} ms with the switch at 2 "
                  f"(the moved launches: {sum(keys[0].values()) / 1e3:.3f} -> {sum(keys[2].values()) / 1e3:.3f} ms)", flush=True)
            rows.append(dict(net=net, batch=batch, summary=True, before_us=round(tot[0], 1), after_us=round(tot[2], 1)))
            del images, out
        del pred
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rows, indent=0))
    if args.write_header:
        write_padded_header(rows, max(batches))


def write_padded_header(rows, batch, hold=96):
    """a row per key (cin_pad, cout_pad, size, kind) that was faster on the tile at `batch` views in every net that has it"""
    won = defaultdict(list)
    for r in rows:
        if not r.get("summary") and r["batch"] == batch:
            won[tuple(r["key"][1:5])].append(r)
    keep = {k: rs for k, rs in won.items() if all(r["faster"] for r in rs)}
    lines = ["// GENERATED by tools/tune_in_network.py --winograd4-padded --write-header on an MI355X: the (shape, kind) keys of the 80- and 84-row",
             "// direct tiles (variants 16 and 26) whose launches ran faster, by more than 2 %, on the F(4,3) Winograd tile over weights padded to",
             "// whole 32-channel columns, timed INSIDE a forward pass.  The dispatcher (conv_mfma.hip: f43_plan) runs such a launch on that tile's",
             "// 32 x 16 workgroup shape over the padded weights.  {cin_pad, cout_pad, size, kind, min_batch}: from min_batch views on.",
             f"// HELD: every row at {hold} views, the correctness gate of conv_tuned_wino4.h (DESIGN 4.1), not a timing result.",
             "#ifndef MVLM_CONV_TUNED_WINO4_PAD_H", "#define MVLM_CONV_TUNED_WINO4_PAD_H",
             "struct ConvTunedWino4Pad {", "    short cin_pad, cout_pad, size, kind, min_batch;", "};",
             "static const ConvTunedWino4Pad MVLM_CONV_TUNED_WINO4_PAD[] = {"]
    for k, rs in sorted(keep.items()):
        note = "; ".join(f"B{batch} {r['launches']} launches: variant {r['direct_variant']} {r['direct_us']} us, padded {r['padded_us']} us [{r['net']}]" for r in rs)
        lines.append(f"    {{{k[0]}, {k[1]}, {k[2]}, {k[3]}, {max(hold, 0)}}},  // {note}")
    lines += ["    {0, 0, 0, 0, 0},  // (end: no layer has zero channels)", "};",
              f"static const int MVLM_CONV_TUNED_WINO4_PAD_N = {len(keep)};", "#endif", ""]
    WINO4_PAD_HEADER.write_text("\n".join(lines))
    print(f"{len(keep)} keys -> {WINO4_PAD_HEADER}")


def write_wide_hold_header(rows, batch):
    """the keys (cin_pad, cout_pad, size, kind) slower on the wide shape at `batch` views in any net, and the rows the header had"""
    import re

    held = {}
    if WIDE_HOLD_HEADER.exists():
        for m in re.finditer(r"^    \{(\d+), (\d+), (\d+), (\d+)\},\s*//(.*)$", WIDE_HOLD_HEADER.read_text(), re.M):
            if int(m.group(1)):  # (not the end row)
                held[tuple(int(v) for v in m.groups()[:4])] = m.group(5).strip()
    for r in rows:
        if not r.get("summary") and r["batch"] == batch and r["slower"]:
            held[tuple(r["key"][1:5])] = f"B{batch} {r['launches']} launches: narrow {r['narrow_us']} us, wide {r['wide_us']} us [{r['net']}]"
    lines = ["// GENERATED by tools/tune_in_network.py --winograd4-wide --write-header on an MI355X: the (shape, kind) keys whose launches on the",
             "// F(4,3) tile ran slower on its wide workgroup shape than on the 32 x 16 shape INSIDE a forward pass, by more than 2 %.  The",
             "// dispatcher (conv_mfma.hip: f43_plan) keeps them on the 32 x 16 shape; every other launch with output channels in 64s takes the wide one.",
             "// {cin_pad, cout_pad, size, kind}",
             "#ifndef MVLM_CONV_WINO4_WIDE_HOLD_H", "#define MVLM_CONV_WINO4_WIDE_HOLD_H",
             "struct ConvWino4WideHold {", "    short cin_pad, cout_pad, size, kind;", "};",
             "static const ConvWino4WideHold MVLM_CONV_WINO4_WIDE_HOLD[] = {"]
    lines += [f"    {{{k[0]}, {k[1]}, {k[2]}, {k[3]}}},  // {note}" for k, note in sorted(held.items())]
    lines += ["    {0, 0, 0, 0},  // (end: no layer has zero channels)", "};",
              f"static const int MVLM_CONV_WINO4_WIDE_HOLD_N = {len(held)};", "#endif", ""]
    WIDE_HOLD_HEADER.write_text("\n".join(lines))
    print(f"{len(held)} keys -> {WIDE_HOLD_HEADER}")


def ap_default_batches():
    return "1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,20,24,32,48,64,96,128"


def write_wino_header(rows, batches, copy_dir=None, four=False, hold=0):
    """entry = the smallest tuned batch from which the key was kept at every tuned batch above it, in every net that has it"""
    kept = defaultdict(dict)  # key -> batch -> (all nets kept, variant, note)
    for r in rows:
        if r.get("summary"):
            continue
        k, b = tuple(r["key"]), r["batch"]
        ok, v, note = kept[k].get(b, (True, r["variant"], ""))
        if b < hold:
            continue
        kept[k][b] = (ok and r["kept"] and v == r["variant"], v, note + f" B{b} {r['direct_us']} -> {r['winograd_us']} us [{r['net']}]")
    sfx, header = ("4", WINO4_HEADER) if four else ("", WINO_HEADER)
    intro = (["// GENERATED by tools/tune_in_network.py --winograd4 --write-header on an MI355X: 3x3 layers that run faster on the F(4,3)",
              "// Winograd tile than on what runs otherwise (the F(2,3) tile, the pair launches or the direct tile), timed INSIDE a forward"] if four else
             ["// GENERATED by tools/tune_in_network.py --winograd --write-header on an MI355X: 3x3 layers that run faster on a Winograd tile",
              "// than on what the direct path launches for them (its pair launches and second-input forms included), timed INSIDE a forward"])
    lines = intro + [
             "// pass of the landmark network.  {cin_pad, cout_pad, size, kind, min_batch, variant}: from min_batch views per device batch on.",
             f"// Tuned at {', '.join(str(b) for b in sorted(batches, reverse=True))} views per device batch ({', '.join(sorted({r['net'] for r in rows}))}): min_batch is the smallest of these from which",
             "// the key won at every tuned batch above it; the note gives the timings at that batch.",
             *([f"// HELD: no row below {hold} views, whatever won there.  For these rows min_batch is a correctness gate, not a timing result:",
                "// the tile also won at smaller tuned batches, but with rows from 12 views on tests/test_gpu_e2e_matrix.py::",
                "// test_planted_peaks_through_the_network (16 views) moved a landmark.  Its detector is made of identity convolutions, which",
                "// this tile's weights g/3, 2g/15, 8g/15 do not copy exactly, and its views' peaks tie up to that rounding.  The rounding is",
                "// the same at every batch; which shapes carry it there was not narrowed down (DESIGN 4.1, profiles/r10_wino4_layers.txt)."] if hold else []),
             f"#ifndef MVLM_CONV_TUNED_WINO{sfx}_H", f"#define MVLM_CONV_TUNED_WINO{sfx}_H",
             f"struct ConvTunedWino{sfx} {{ short cin_pad, cout_pad, size, kind, min_batch, variant; }};",
             f"static const ConvTunedWino{sfx} MVLM_CONV_TUNED_WINO{sfx}[] = {{"]
    n = 0
    for k in sorted(kept):
        min_batch, variant, note = None, None, ""
        for b in sorted(kept[k], reverse=True):
            ok, v, nt = kept[k][b]
            if not ok or (variant is not None and v != variant):
                break
            min_batch, variant, note = b, v, nt
        if min_batch is not None:
            lines.append(f"    {{{k[1]}, {k[2]}, {k[3]}, {k[4]}, {min_batch}, {variant}}},  //{note}")
            n += 1
    if n == 0:
        lines.append("    {0, 0, 0, 0, 0, -1},")
    lines += ["};", f"static const int MVLM_CONV_TUNED_WINO{sfx}_N = {n};", "#endif", ""]
    header.write_text("\n".join(lines))
    if copy_dir is not None:  # a copy beside the tuner's JSON (--out)
        Path(copy_dir).mkdir(parents=True, exist_ok=True)
        (Path(copy_dir) / header.name).write_text("\n".join(lines))
    print(f"wrote {header} ({n} entries)")


def write_header(rows, merge=False):
    lines = ["// GENERATED by tools/tune_in_network.py --write-header on an MI355X: kernel variant per (layer shape, kind, device batch),",
             "// every candidate timed INSIDE a forward pass of the landmark network on real activations (HIP events per launch).",
             "// {ksize, cin_pad, cout_pad, size, kind, batch, variant}; kind 0 plain / residual-block layer, 1 scatter into the skip tensor,",
             "// 2 pooled output wanted; sorted; the dispatcher uses the entry of the smallest tuned batch >= the launch's batch.",
             "#ifndef MVLM_CONV_TUNED_NET_H", "#define MVLM_CONV_TUNED_NET_H",
             "struct ConvTunedNet { short ksize, cin_pad, cout_pad, size, kind, batch, variant; };",
             "static const ConvTunedNet MVLM_CONV_TUNED_NET[] = {"]
    import re

    table = {}
    if merge and HEADER.exists():
        for m in re.finditer(r"^    \{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (-?\d+)\},\s*// (.*)$", HEADER.read_text(), re.M):
            table[tuple(int(m[i]) for i in range(1, 7))] = (int(m[7]), m[8])
    for r in rows:
        if r.get("summary"):
            continue
        # (every tuned key is listed, changed or not: the dispatcher takes the entry of the smallest tuned batch >= B, so a key
        #  missing at one batch would inherit another batch's winner)
        kept_name = r["best_name"] if r["kept"] == r["best"] else r["current_name"]
        note = f"{kept_name} {r['best_us'] if r['kept'] == r['best'] else r['current_us']} us"
        if r["kept"] != r["current"]:
            note += f" (was {r['current_name']} {r['current_us']} us)"
        table[tuple(r["key"]) + (r["batch"],)] = (r["kept"], note + f" [{r['net']}]")
    for k in sorted(table):
        v, note = table[k]
        lines.append(f"    {{{k[0]}, {k[1]}, {k[2]}, {k[3]}, {k[4]}, {k[5]}, {v}}},  // {note}")
    n = sum(1 for ln in lines if ln.startswith("    {"))
    if n == 0:
        lines.append("    {0, 0, 0, 0, 0, 0, -1},")
    lines += ["};", f"static const int MVLM_CONV_TUNED_NET_N = {n};", "#endif", ""]
    HEADER.write_text("\n".join(lines))
    (REPO / "gpurun_out" / "conv_tuned_net.h").write_text("\n".join(lines))
    print(f"wrote {HEADER} ({len(table)} entries)")


if __name__ == "__main__":
    main()
