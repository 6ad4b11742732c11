"""No GPU: the result buffer's one layout (utils/report.py: ResultPack), the ray selection (utils/viewer.py: select_rays), the
finite-landmark filter of the pictures (pipeline/pictures.py) and what general_pipeline.py no longer writes out by hand."""
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
PIPELINE_SRC = REPO / "mvlm_amd" / "pipeline" / "general_pipeline.py"


@pytest.mark.parametrize("nl", (1, 3, 73, 84, 478))   # 36 nl is no multiple of 8 for 1, 3 and 73; 84 and 478 are the product's counts
def test_result_pack_has_the_hand_written_offsets(nl):
    from mvlm_amd.utils.report import ReportLayout, ResultPack

    rp = ResultPack(nl)
    assert [rp.fields[k][:2] for k in ("snapped", "error", "counts")] == [(0, 24 * nl), (24 * nl, 8 * nl), (32 * nl, 4 * nl)]
    assert rp.fields["counts"][0] + rp.fields["counts"][1] == 36 * nl
    assert rp.nbytes == (36 * nl + 7) // 8 * 8 and rp.total == rp.nbytes and rp.report is None   # nbytes: the group stride too
    for n in (1, 8):
        with_report = ResultPack(nl, n)
        assert with_report.fields == rp.fields and with_report.nbytes == rp.nbytes
        assert with_report.report.nbytes == ReportLayout(nl, n).nbytes and (with_report.report.nl, with_report.report.n) == (nl, n)
        assert with_report.total == rp.nbytes + ReportLayout(nl, n).nbytes
        buf = np.arange(with_report.total + 16, dtype=np.uint64).astype(np.uint8)
        got = with_report.report_bytes(buf)                       # the report starts at the rounded size
        assert got.size == ReportLayout(nl, n).nbytes and np.shares_memory(got, buf) and got[0] == buf[rp.nbytes]


@pytest.mark.parametrize("nl", (1, 3, 73, 84, 478))
def test_result_pack_views_alias_the_buffer_on_both_sides(nl):
    import torch

    from mvlm_amd.utils.report import ResultPack

    rp = ResultPack(nl)
    rs = np.random.RandomState(nl)
    snapped, error, counts = rs.normal(size=(nl, 3)), rs.uniform(size=nl), rs.randint(0, 96, nl).astype(np.int32)
    raw = np.zeros(rp.nbytes + 8, np.uint8)                       # (a buffer longer than the pack, as a reused one is)
    raw[: 24 * nl] = snapped.view(np.uint8).ravel()               # written by hand, at the hand-written offsets
    raw[24 * nl: 32 * nl] = error.view(np.uint8)
    raw[32 * nl: 36 * nl] = counts.view(np.uint8)
    buf = torch.from_numpy(raw.copy())
    dev, host = rp.device_views(buf), rp.host_views(raw)
    assert list(dev) == list(host) == ["snapped", "error", "counts"]
    for name, want in (("snapped", snapped), ("error", error), ("counts", counts)):
        assert tuple(dev[name].shape) == host[name].shape == want.shape
        assert host[name].dtype == want.dtype and dev[name].numpy().dtype == want.dtype
        np.testing.assert_array_equal(host[name], want)
        np.testing.assert_array_equal(dev[name].numpy(), want)
        assert np.shares_memory(host[name], raw) and dev[name].data_ptr() == buf.data_ptr() + rp.fields[name][0]
    # writing through a view changes the bytes, on both sides
    dev["counts"][nl - 1] = 77
    host["counts"][nl - 1] = 77
    dev["snapped"][0, 2] = -1.5
    host["snapped"][0, 2] = -1.5
    for changed in (buf.numpy(), raw):
        assert changed[36 * nl - 4: 36 * nl].view(np.int32)[0] == 77 and changed[16:24].view(np.float64)[0] == -1.5
    np.testing.assert_array_equal(buf.numpy(), raw)


def test_select_rays():
    from mvlm_amd.utils.viewer import select_rays

    assert select_rays(4, 8) == ([0, 1, 2, 3], list(range(8)))                 # None: all
    assert select_rays(8, 8, [0, 5, -1], None) == ([0, 5, 7], list(range(8)))
    assert select_rays(8, 3, None, [3, 4, 10, -4]) == (list(range(8)), [0, 1, 1, 2])   # n or more wraps round
    assert select_rays(8, 3, [], []) == ([], [])                               # an empty list stays empty
    assert select_rays(8, 3, np.array([1.0, 9]), (np.int64(2),)) == ([1, 1], [2])


def test_the_call_sites_select_what_np_ix_selects(tmp_path):
    import torch

    from mvlm_amd.pipeline import DTU3DPipeline
    from mvlm_amd.utils.viewer import select_rays

    rs = np.random.RandomState(0)
    starts, ends = rs.normal(size=(8, 5, 3)), rs.normal(size=(8, 5, 3))
    lm, views = [0, 5, -1], [1, 7]
    want_rows, want_cols = [0, 5, 7], [1, 2]
    # dump_rays, unclipped: host work only
    pipe = object.__new__(DTU3DPipeline)
    pipe.__dict__.update(_rays=(None, starts, ends), screenshot_folder=tmp_path, verbose=False)
    dump = np.load(pipe.dump_rays("scan.obj", np.zeros((8, 3)), lm, views, clip_to_mesh=False))
    np.testing.assert_array_equal(dump["starts"], starts[np.ix_(want_rows, want_cols)])
    np.testing.assert_array_equal(dump["ends"], ends[np.ix_(want_rows, want_cols)])
    assert dump["landmark_indices"].tolist() == want_rows and dump["view_indices"].tolist() == want_cols
    # the ray view's two index_select calls over the same lists
    li, vi = (torch.as_tensor(x, dtype=torch.long) for x in select_rays(8, 5, lm, views))
    np.testing.assert_array_equal(torch.from_numpy(starts).index_select(0, li).index_select(1, vi).numpy(), starts[np.ix_(want_rows, want_cols)])
    # and nobody wraps an index on their own: the ray view, the dump and RayVisualizer.show all go through select_rays
    sources = [PIPELINE_SRC, PIPELINE_SRC.with_name("pictures.py"), REPO / "mvlm_amd" / "utils" / "viewer.py"]
    assert [p.read_text().count("[int(i) %") for p in sources] == [0, 0, 2]    # (both in select_rays)
    assert all("select_rays(" in p.read_text() for p in sources)
    assert (REPO / "mvlm_amd" / "utils" / "viewer.py").read_text().count("select_rays(") == 2   # its definition and show


def test_the_finite_filter():
    from mvlm_amd.pipeline.pictures import finite_landmarks

    landmarks = np.arange(12, dtype=np.float64).reshape(4, 3)
    colours = np.arange(12, dtype=np.uint8).reshape(4, 3)
    got, got_colours = finite_landmarks(landmarks, colours)
    assert np.shares_memory(got, landmarks) and got.shape == (4, 3) and got_colours is colours   # all finite: the inputs, no copy
    np.testing.assert_array_equal(got, landmarks)
    assert finite_landmarks(landmarks)[1] is None
    bad = landmarks.copy()
    bad[2, 1] = np.nan
    got, got_colours = finite_landmarks(bad, colours)
    np.testing.assert_array_equal(got, landmarks[[0, 1, 3]])
    np.testing.assert_array_equal(got_colours, colours[[0, 1, 3]])
    bad[0, 0] = np.inf
    got, got_colours = finite_landmarks(bad.ravel().tolist(), None)             # anything that reshapes to [NL,3]; no colours
    np.testing.assert_array_equal(got, landmarks[[1, 3]])
    assert got_colours is None


def test_the_pipeline_writes_no_offsets_and_no_rule_of_its_own():
    src = PIPELINE_SRC.read_text()
    for literal in ("* 24", "* 32", "* 36"):
        assert literal not in src, literal
    rule = "needs a HipRenderer3D in the renderer slot"
    assert src.count(rule) == 0 and PIPELINE_SRC.with_name("pictures.py").read_text().count(rule) == 1
