"""The pictures a prediction can leave behind: their options' checks, their rules, and the one hook that draws them.

The options are plain attributes of ``Pipeline``; every function here takes the pipeline.  All of them are off by default, and
then nothing of them is launched, allocated or copied.  A failed prediction (no landmarks) draws nothing.

visualize_img       the RESIDENT device mesh with a sphere at every landmark (the reference's --visualize-img, main.py:66-67;
                    HipRenderer3D.render_landmark_view) into visualization/<stem>_<visualize_name>.png under the working
                    directory, visualize_size pixels a side.  With landmark_report the spheres carry the report's branch
                    colours (utils/report.py: BRANCH_COLOURS).
visualize_rays_img  the resident mesh with every selected view ray (the device tensors the consensus just used, clipped on the
                    device when clip_rays_to_mesh is set) and the landmarks, one picture per pose of visualize_rays_poses in ONE
                    call (the reference's visualize_rays=True, visualization/ray_visualizer.py; HipRenderer3D.render_ray_view),
                    into <screenshot_folder or visualization/ray_screenshots>/<stem>_<visualize_name>_rays_<i>.png.  With
                    landmark_report the rays carry LandmarkReport.ray_colours().  A flag of its own: visualize_rays keeps
                    writing its .npz and nothing else.  Drawn by _after_prediction, which knows the file and the selection:
                    predict_mesh_device called on its own has no file name, draws nothing and leaves nothing behind.
visualize_sheet     the views the network saw, side by side, with a marker where it put each landmark in each view and a red
                    residual to where the final landmark projects there (the reference's Predictor2D.draw_image_with_landmarks
                    for all views; HipRenderer3D.render_view_sheet), from this pass's own device buffers, into
                    visualization/<stem>_<visualize_name>_views.png; sheet_scale 1..4 sheet pixels per view pixel.  With
                    landmark_report a view the score filter dropped gets a ring and the markers carry the branch colours.
visualize_heat      the view sheet's cells, no markers, with the network's heatmaps laid over them: per pixel the landmark (of
                    heat_landmarks; None: all) whose value is the largest share of its plane's peak, in its colour of
                    utils/viewer.py's palette, shares up to heat_floor not drawn (HipRenderer3D.render_heat_sheet), into
                    visualization/<stem>_<visualize_name>_heat.png; sheet_scale applies as for the view sheet.  The heatmaps are
                    not kept by the prediction: the predictor's heatmaps_device runs once more on this pass's image stack, which
                    costs about one network pass more per scan, and its tensor ([N,NL,256,256] float32: 2 GB at 96 views x 84
                    landmarks) lives until the picture is drawn.
visualize_surface   all views' heatmaps laid on the scan itself (HipRenderer3D.surface_heat): every vertex takes, from every view that
                    sees it (at most surface_depth_tol depth steps behind that view's depth plane), the share its heatmap value there
                    has of its plane's peak; the mesh is drawn with the winning landmark's colour per vertex - heat_landmarks and
                    heat_floor as for the heat sheet - and the final landmarks as spheres, front view, frame="fit", visualize_size
                    pixels a side, into visualization/<stem>_<visualize_name>_surface.png.  It leaves last_surface_path and
                    last_surface_heat = {peak_vertex, peak_score, distance}: per landmark the vertex where the views together put
                    it, its score, and the distance from there to the final landmark (NaN where either is missing) - a second
                    opinion beside rays + RANSAC.  Costs the heat sheet's second network pass; with visualize_heat as well the
                    heatmaps are made once for both pictures.
view_png_encoder    who makes the PNG files.  "host" (the default): the picture is copied to the host and Pillow encodes it.
                    "device": it stays where render_*_device left it and HipRenderer3D.encode_png filters and compresses it there
                    (mvlm_png_encode; the ray view's pictures in one call) - the same pixels in a file of other bytes, and only
                    the compressed bytes cross to the host.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path

import numpy as np

from .. import parallel
from ..utils.render3d import HipRenderer3D
from ..utils.report import LandmarkReport
from ..utils.viewer import heat_colours, heat_sheet_path, render_to_png, select_rays, surface_path, view_path, view_sheet_path

FLAGS = ("visualize_heat", "visualize_surface", "visualize_sheet", "visualize_rays_img", "visualize_img")  # in the order their rules are checked
SHEETS = ("visualize_heat", "visualize_sheet")  # they draw the views
ALL_VIEWS = SHEETS + ("visualize_surface",)  # they read every view, and need them all in one process
HEATMAPS = ("visualize_heat", "visualize_surface")  # they show the network's heatmaps


@dataclass
class Pass:
    """What one pass left behind, as the pictures need it: device tensors on the fused path, numpy arrays on the slot path.
    ``images`` [N,256,256,4], ``maxima`` [NL,N,3], ``rot`` and the rays ``starts`` / ``ends`` [NL,N,3] hold the views a detector's
    ``valid`` mask left; ``landmarks`` are in the space the mesh was uploaded in (with a pre-align block: before the inverse
    mapping, so the points sit on the drawn surface); ``report``: THIS pass's LandmarkReport or None; ``draws``: whether this rank
    draws what every rank could (sharded, every rank holds the result and one draws)."""
    mesh: object
    images: object
    maxima: object
    rot: object
    starts: object
    ends: object
    landmarks: object
    report: object = None
    draws: bool = True


def wanted(pipe) -> bool:
    """Does the pass now running have a picture to draw (or rays to keep for one)?"""
    return pipe.visualize_img or pipe.visualize_sheet or pipe.visualize_heat or pipe.visualize_surface or pipe._keep_ray_view


def keeps_images(pipe) -> bool:
    """Does a picture of the pass now running read the image stack behind the prediction?"""
    return pipe.visualize_sheet or pipe.visualize_heat or pipe.visualize_surface


def check_options(pipe, n_views, heat_landmarks, visualize_size) -> None:
    """The constructor's checks of the picture options, which it has assigned as given; leaves ``sheet_scale``, ``heat_floor``
    and ``heat_landmarks`` in their checked form."""
    scale, floor = pipe.sheet_scale, pipe.heat_floor
    if pipe.visualize_sheet or pipe.visualize_heat:
        if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or not 1 <= scale <= 4:
            raise ValueError(f"sheet_scale must be an integer in 1..4, not {scale!r}")
        pipe.sheet_scale = int(scale)
    if pipe.visualize_sheet and n_views is not None:  # (a sheet beyond 4096 pixels a side: said here, with the scale that fits)
        HipRenderer3D.view_sheet_layout(int(n_views), None, pipe.sheet_scale)
    if pipe.visualize_surface:
        tol = pipe.surface_depth_tol
        if isinstance(tol, bool) or not isinstance(tol, (int, np.integer)) or not 0 <= tol <= 255:
            raise ValueError(f"surface_depth_tol must be an integer in 0..255, not {tol!r}")
        pipe.surface_depth_tol = int(tol)
    if pipe.visualize_heat or pipe.visualize_surface:
        if isinstance(floor, bool) or not isinstance(floor, (int, float, np.integer, np.floating)) \
                or not (np.isfinite(floor) and 0.0 <= floor < 1.0):
            raise ValueError(f"heat_floor must be a finite number in [0, 1), not {floor!r}")
        pipe.heat_floor = float(floor)
        if heat_landmarks is not None:
            picked = list(heat_landmarks) if isinstance(heat_landmarks, (list, tuple, range, np.ndarray)) else None
            if picked is None or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0 for k in picked) \
                    or len(set(int(k) for k in picked)) != len(picked):
                raise ValueError(f"heat_landmarks must be None or a sequence of distinct landmark indices, not {heat_landmarks!r}")
            pipe.heat_landmarks = [int(k) for k in picked]  # (the upper end: check(), once the predictor is there)
        if pipe.visualize_heat and n_views is not None:  # (as for the view sheet)
            HipRenderer3D._sheet_layout("heat sheet", int(n_views), None, pipe.sheet_scale, 2)
    size = pipe.visualize_size
    if (pipe.visualize_img or pipe.visualize_rays_img or pipe.visualize_surface) and (size < 64 or size > 2048 or size % 16):
        raise ValueError(f"visualize_size must be a multiple of 16 in 64..2048, not {visualize_size}")


def check(pipe) -> None:
    """The rules of ``Pipeline._check_visualize``, said before the prediction, not after it: every picture needs the renderer that
    holds the mesh on the device and draws; the sheets need all the views in one process; the heat sheet needs a predictor that
    hands out its heatmaps, and landmarks that predictor has."""
    for flag in FLAGS:
        if not getattr(pipe, flag):
            continue
        reason = "it draws the sheet" if flag in SHEETS else "it draws the mesh resident on the device"
        if flag in HEATMAPS and not callable(getattr(pipe.predictor_2d, "heatmaps_device", None)):
            raise ValueError(f"{flag} needs a predictor with heatmaps_device (HipPaulsenModel): "
                             f"{type(pipe.predictor_2d).__name__} has no heatmaps to show")
        if not isinstance(pipe.renderer_3d, HipRenderer3D):
            raise ValueError(f"{flag} needs a HipRenderer3D in the renderer slot ({reason}), not {type(pipe.renderer_3d).__name__}")
        if flag in ALL_VIEWS and pipe.shard_views and parallel.is_distributed():
            raise ValueError(f"{flag} is not supported with shard_views in a distributed run: a rank holds only its slice of the views")
        if flag in HEATMAPS and pipe.heat_landmarks is not None:
            nl = int(pipe.predictor_2d.get_lm_count())
            if any(k >= nl for k in pipe.heat_landmarks):
                raise ValueError(f"heat_landmarks must lie in 0..{nl - 1}, not {pipe.heat_landmarks!r}")


def finite_landmarks(landmarks, colours=None) -> tuple:
    """(landmarks f64 [NL,3], their colour rows or None) without the landmarks that are not finite (a consensus without lines can
    leave one): a picture flag does not fail a prediction that succeeded."""
    landmarks = np.asarray(landmarks, dtype=np.float64).reshape(-1, 3)
    finite = np.isfinite(landmarks).all(axis=1)
    if not finite.all():
        landmarks = landmarks[finite]
        colours = None if colours is None else colours[finite]
    return landmarks, colours


def _mesh_name(mesh):
    return getattr(mesh, "path", None) or "mesh.obj"


def _sheet_look(pipe) -> dict:
    """What both sheets share: the background is the planes the predictor read."""
    return dict(background="auto", scale=pipe.sheet_scale, chan_sel=getattr(pipe.predictor_2d, "chan_sel", None))


def draw_landmark_view(pipe, mesh, landmarks, report=None):
    """``visualize_img``: the mesh as it lies on the device - no second ingest, no second upload -, front view, ``frame="fit"``;
    written as ``LandmarkViewer`` names it.  ``report``'s branches colour the spheres (None: blue)."""
    if landmarks is None:
        return None
    with pipe._timer.stage("visualize"):
        landmarks, colours = finite_landmarks(landmarks, report.branch_colours() if report is not None else None)
        _, pipe.last_view_path = render_to_png(pipe.renderer_3d, "landmark_view", pipe.view_png_encoder,
                                               view_path(_mesh_name(mesh), pipe.visualize_name), mesh, landmarks, first=True,
                                               size=pipe.visualize_size, colors=colours)
    pipe._say(f"[Pipeline] landmark view written to {pipe.last_view_path}")
    return pipe.last_view_path


def draw_view_sheet(pipe, p: Pass):
    """``visualize_sheet``: ``HipRenderer3D.render_view_sheet`` of the pass; the report's survivor flags make rings, its branches
    colour the markers."""
    with pipe._timer.stage("visualize_sheet"):
        colours = used = None
        if p.report is not None:
            colours = p.report.branch_colours()
            used = ((np.asarray(p.report.view_flags) & LandmarkReport.VIEW_KEPT) != 0).astype(np.uint8)
        # (a detector's device maxima may be float64; the network's are float32 already)
        maxima = p.maxima.float() if hasattr(p.maxima, "data_ptr") else p.maxima
        _, pipe.last_sheet_path = render_to_png(
            pipe.renderer_3d, "view_sheet", pipe.view_png_encoder, view_sheet_path(_mesh_name(p.mesh), pipe.visualize_name), p.images,
            maxima=maxima, rot=p.rot, landmarks=np.asarray(p.landmarks, dtype=np.float64).reshape(-1, 3), colors=colours, used=used,
            **_sheet_look(pipe))
    pipe._say(f"[Pipeline] view sheet written to {pipe.last_sheet_path}")


def pass_heatmaps(pipe, p: Pass) -> tuple:
    """(the pass's image stack on the device, the heatmaps the predictor makes of it - a second forward pass): made once per pass,
    for the heat sheet and the surface heat alike."""
    import torch

    images = p.images
    if not hasattr(images, "data_ptr"):
        images = torch.from_numpy(np.ascontiguousarray(images, dtype=np.float32)).to(torch.device("cuda", pipe.renderer_3d.ctx.device))
    return images, pipe.predictor_2d.heatmaps_device(images)


def draw_heat_sheet(pipe, p: Pass, images, heat):
    """``visualize_heat``: the views of the pass with the heatmaps the predictor made of them (``pass_heatmaps``), drawn by
    ``HipRenderer3D.render_heat_sheet``."""
    with pipe._timer.stage("visualize_heat"):
        _, pipe.last_heat_path = render_to_png(
            pipe.renderer_3d, "heat_sheet", pipe.view_png_encoder, heat_sheet_path(_mesh_name(p.mesh), pipe.visualize_name), images, heat,
            landmarks=pipe.heat_landmarks, colors=heat_colours(int(heat.shape[1])), floor=pipe.heat_floor, **_sheet_look(pipe))
    pipe._say(f"[Pipeline] heat sheet written to {pipe.last_heat_path}")


def draw_surface_heat(pipe, p: Pass, images, heat):
    """``visualize_surface``: the heatmaps of the pass laid on the resident mesh (``HipRenderer3D.surface_heat``), the mesh drawn
    with those colours and the final landmarks as spheres (the report's branch colours, else blue).  Leaves ``last_surface_path``,
    ``last_surface_heat`` and, for ``write_surface_mesh``, the mesh and its colours on the device."""
    with pipe._timer.stage("visualize_surface"):
        r3 = pipe.renderer_3d
        nl = int(heat.shape[1])
        res = r3.surface_heat(p.mesh, images, heat, np.asarray(p.rot, dtype=np.float64), landmarks=pipe.heat_landmarks,
                              colors=heat_colours(nl), floor=pipe.heat_floor, depth_tol=pipe.surface_depth_tol)
        landmarks, colours = finite_landmarks(p.landmarks, p.report.branch_colours() if p.report is not None else None)
        _, pipe.last_surface_path = render_to_png(r3, "landmark_view", pipe.view_png_encoder,
                                                  surface_path(_mesh_name(p.mesh), pipe.visualize_name), p.mesh, landmarks, first=True,
                                                  size=pipe.visualize_size, colors=colours, vertex_colors=res["colors"])
        peak_vertex = res["peak_vertex"].cpu().numpy()
        final = np.asarray(p.landmarks, dtype=np.float64).reshape(-1, 3)
        distance = np.full(nl, np.nan)
        found = np.nonzero(peak_vertex >= 0)[0]
        found = found[found < len(final)]
        at = np.asarray(p.mesh.verts, dtype=np.float64).reshape(-1, 3)[peak_vertex[found]]
        distance[found] = np.linalg.norm(final[found] - at, axis=1)  # (NaN where the final landmark is not finite)
        pipe.last_surface_heat = {"peak_vertex": peak_vertex, "peak_score": res["peak_score"].cpu().numpy(), "distance": distance}
        pipe._surface_mesh = (p.mesh, res["colors"])
    pipe._say(f"[Pipeline] surface heat written to {pipe.last_surface_path}")


def write_surface_mesh(pipe, path) -> Path:
    """The mesh of the last ``visualize_surface`` picture with its colours as an OBJ with per-vertex colours (``write_obj``): only
    the V x 4 colour bytes cross from the device."""
    from ..utils.mesh_io import write_obj

    if getattr(pipe, "_surface_mesh", None) is None:
        raise ValueError("write_surface_mesh: no surface heat has been drawn (visualize_surface)")
    mesh, colours = pipe._surface_mesh
    path = Path(path)
    write_obj(path, np.asarray(mesh.verts), np.asarray(mesh.tris), colors=colours.cpu().numpy()[:, :3])
    return path


def draw_ray_view(pipe, p: Pass, file_name, landmark_indices=None, view_indices=None, clip_to_mesh: bool = True):
    """``visualize_rays_img``: the pictures the reference's ``RayVisualizer`` shows (ray_visualizer.py:150-338) - the rays of the
    selected landmarks and views (subset exactly as ``Pipeline.dump_rays`` subsets them) from the tensors the consensus used,
    clipped on the device; all poses in one call.  Returns the paths (also ``last_ray_view_paths``)."""
    import torch

    with pipe._timer.stage("visualize_rays"):
        dev = torch.device("cuda", pipe.renderer_3d.ctx.device)
        starts, ends = (x if hasattr(x, "data_ptr") else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
                        for x in (p.starts, p.ends))
        lm_idx, v_idx = select_rays(int(starts.shape[0]), int(starts.shape[1]), landmark_indices, view_indices)
        li = torch.as_tensor(lm_idx, dtype=torch.long, device=dev)
        vi = torch.as_tensor(v_idx, dtype=torch.long, device=dev)
        fs = starts.index_select(0, li).index_select(1, vi).contiguous()
        fe = ends.index_select(0, li).index_select(1, vi).contiguous()
        if clip_to_mesh and fs.numel():
            fe, _ = pipe.estimator_3d.clip_rays_device(p.mesh, fs, fe)
        colours = ray_colours = None
        if p.report is not None:
            colours = p.report.branch_colours()
            ray_colours = p.report.ray_colours(np.asarray(p.report.view_indices)[v_idx])[lm_idx].reshape(-1, 3)
        landmarks, colours = finite_landmarks(p.landmarks, colours)
        folder = Path(pipe.screenshot_folder) if pipe.screenshot_folder else Path.cwd() / "visualization" / "ray_screenshots"
        paths = [folder / f"{Path(file_name).stem}_{pipe.visualize_name}_rays_{i}.png" for i in range(len(pipe.visualize_rays_poses))]
        _, pipe.last_ray_view_paths = render_to_png(pipe.renderer_3d, "ray_view", pipe.view_png_encoder, paths, p.mesh, landmarks, fs, fe,
                                                    poses=pipe.visualize_rays_poses, size=pipe.visualize_size, colors=colours,
                                                    ray_colors=ray_colours)
    pipe._say(f"[Pipeline] ray view written to {[str(q) for q in pipe.last_ray_view_paths]}")
    return pipe.last_ray_view_paths


def draw(pipe, p: Pass) -> None:
    """The one hook both paths call behind a prediction: landmark view, view sheet, heat sheet, surface heat, in this order, and the pass kept
    for the ray view, which ``_after_prediction`` draws."""
    check(pipe)
    if p.landmarks is not None:
        if pipe.visualize_img and p.draws:
            pipe._draw_landmark_view(p.mesh, p.landmarks, p.report)
        if pipe.visualize_sheet and p.images is not None:
            draw_view_sheet(pipe, p)
        if (pipe.visualize_heat or pipe.visualize_surface) and p.images is not None:
            images, heat = pass_heatmaps(pipe, p)  # once, for both pictures
            if pipe.visualize_heat:
                draw_heat_sheet(pipe, p, images, heat)
            if pipe.visualize_surface and p.draws:
                draw_surface_heat(pipe, p, images, heat)
    if pipe._keep_ray_view and p.draws:
        pipe._ray_view = p
