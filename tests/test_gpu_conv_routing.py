"""-m gpu: the kernel variant every convolution launch of a forward pass runs on, against tests/golden/conv_slot_variants.json.

Seven launch-by-launch passes of the 84-landmark RGB+depth network with synthetic weights: device batches 1, 2 and 12 in Winograd
modes 0 and 1 at the default pairing, and batch 2 in mode 1 with pairing off.  Each pass's profile is its list of
(conv slot, variant id) in launch order (slot -1: the pool kernel; a paired launch: the first problem's slot and the pair's
variant code).  The assertion is that the network launches the same kernels as when the golden was recorded; the arithmetic
is the parity tests' business.

The golden is a function of the committed tuned tables (conv_tuned*.h, conv_pair_tuned.h): a retune regenerates it, by this
test with MVLM_WRITE_CONV_SLOT_VARIANTS=1 in the environment."""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import REPO, seeded_images

pytestmark = pytest.mark.gpu

GOLDEN = REPO / "tests/golden/conv_slot_variants.json"
CAP = 1024
PASSES = [(w, 1, b) for w in (0, 1) for b in (1, 2, 12)] + [(1, 0, 2)]   # Winograd mode, pairing, device batch


def _profile(pred, x):
    ctx = pred.ctx
    ctx.check(ctx.lib.mvlm_cnn_set_profiling(ctx.handle, 1))
    try:
        pred.predict_device(x)
        slot, var = (C.c_int32 * CAP)(), (C.c_int32 * CAP)()
        fl, ms = (C.c_double * CAP)(), (C.c_float * CAP)()
        n = ctx.lib.mvlm_cnn_get_profile(ctx.handle, slot, var, fl, ms, CAP)
        assert 0 < n < CAP
        return [[slot[i], var[i]] for i in range(n)]
    finally:
        ctx.check(ctx.lib.mvlm_cnn_set_profiling(ctx.handle, 0))


def test_the_network_launches_the_recorded_kernel_variants():
    from mvlm_amd.prediction import BU3DFEPredictor

    pred = BU3DFEPredictor(image_mode="RGB+depth", weights="synthetic:6", verbose=False)
    ctx = pred.ctx
    images = torch.from_numpy(seeded_images(9, 12)).cuda()
    got = {}
    try:
        for wino, pairing, batch in PASSES:
            ctx.check(ctx.lib.mvlm_cnn_set_winograd(ctx.handle, wino))
            pred.set_execution(graphs=False, pairing=pairing)
            got[f"winograd{wino}_pairing{pairing}_batch{batch}"] = _profile(pred, images[:batch].contiguous())
    finally:
        ctx.check(ctx.lib.mvlm_cnn_set_winograd(ctx.handle, 1))
        pred.set_execution(graphs=True, pairing=1)
    if os.environ.get("MVLM_WRITE_CONV_SLOT_VARIANTS") == "1":
        GOLDEN.write_text("{\n" + ",\n".join(f'  "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in got.items()) + "\n}\n")
    want = json.loads(GOLDEN.read_text())
    assert sorted(got) == sorted(want)
    for key in got:
        assert len(got[key]) > 80, (key, len(got[key]))
        differ = [(i, g, w) for i, (g, w) in enumerate(zip(got[key], want[key])) if g != w]
        assert not differ and len(got[key]) == len(want[key]), (key, len(got[key]), len(want[key]), differ[:8])
