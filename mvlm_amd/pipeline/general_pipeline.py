"""``Pipeline.predict_one_file`` - the hot path's orchestrator.

Same class surface as the reference's ``Pipeline``
(src/mvlm/pipeline/general_pipeline.py:39-146): constructor kwargs, the three
duck-typed slots ``renderer_3d`` / ``predictor_2d`` / ``estimator_3d``,
``get_lm_count`` and ``predict_one_file(file_name, landmark_indices=None,
view_indices=None, clip_rays_to_mesh=True) -> ndarray[NL,3] | None``.

When all three slots are this package's HIP objects the call runs *fused*: the
rendered views, the maxima and the rays never leave HBM; only the per-landmark
survivor counts (for the host-side RANSAC draw) and the final [NL,3] result cross
PCIe.  Any other object in a slot (a user predictor, the reference's own classes)
is driven through the reference's numpy slot protocol instead.
"""
from __future__ import annotations

import abc
import functools
import os
import threading
import time
from pathlib import Path

import numpy as np

from .. import parallel
from ..prediction.paulsenpredictor import HipPaulsenModel
from ..utils.estimator3d import HipEstimator3D
from ..utils.hostmem import retain_freed_host_memory
from ..utils.render3d import HipRenderer3D
from ..utils.report import LandmarkReport, ResultPack
from ..utils.viewer import check_png_encoder, select_rays
from . import pictures

__all__ = ["Pipeline"]


def _serialised(method):
    """One caller at a time per pipeline.  The reference's server calls ``predict_one_file`` from a thread pool
    without locks (3DMD_server.py:26-31); here a call owns the pipeline's device buffers (image stack, maxima,
    result pack), its captured launch graphs, ``timings`` and the per-call ray state, so the whole call - RNG
    draws included - runs under the pipeline's re-entrant lock."""
    @functools.wraps(method)
    def locked(self, *args, **kwargs):
        with self._lock:
            return method(self, *args, **kwargs)
    return locked


def _drop(box: list) -> None:
    """Release the last reference to whatever ``box`` holds on the calling (reader) thread."""
    box.clear()


class StageTimer:
    """Wall-clock seconds per stage of the last call, under the reference's stage names
    (the reference prints them through tic/toc, general_pipeline.py:84-111; here they are kept
    as a dict so callers and bench.py can read them, and printed in the same wording when verbose)."""

    LABELS = {"render": "Render [Total]: ", "prediction": "Prediction [Total]: ",
              "lines": "Landmarks [0] - From Heatmaps: ", "consensus": "Landmarks [1] - From View Lines: ",
              "project": "Landmarks [2] - Project to Surface: ", "total": "Landmarks 3D Total: "}

    def __init__(self, sink: dict, say):
        self.sink, self.say = sink, say

    @staticmethod
    def fmt(seconds: float) -> str:
        return f"{seconds:08.6f} s"

    def stage(self, name: str):
        return _Stage(self, name)


class _Stage:
    def __init__(self, timer: StageTimer, name: str):
        self.timer, self.name = timer, name

    def __enter__(self):
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        dt = time.perf_counter() - self.t0
        self.timer.sink[self.name] = dt
        if exc[0] is None:
            self.timer.say(StageTimer.LABELS.get(self.name, self.name + ": "), StageTimer.fmt(dt))
        return False


class Pipeline(abc.ABC):
    # (also for an object that never went through __init__: the picture rules and predict_mesh_device read them)
    visualize_heat = visualize_surface = _keep_ray_view = False
    heat_landmarks = None
    point_surface = "splats"
    landmark_distances = False
    distance_pairs = None

    def __init__(self, render_image_stack: bool = False, offscreen: bool = True, n_views: int = 8,
                 render_image_folder: Path | None = None, visualize_rays: bool = False,
                 screenshot_folder: Path | None = None, device: int = 0, shard_views: bool = False,
                 verbose: bool = True, render_multisamples: int = 0, landmark_report: bool = False,
                 visualize_img: bool = False, visualize_size: int = 1024, visualize_name: str | None = None,
                 visualize_rays_img: bool = False, visualize_rays_poses=((0, 0, 0), (0, 60, 0), (0, -60, 0)),
                 view_png_encoder: str = "host", point_radius: float | None = None, visualize_sheet: bool = False,
                 sheet_scale: int = 1, visualize_heat: bool = False, heat_landmarks=None, heat_floor: float = 0.25,
                 point_normals: str = "file", visualize_surface: bool = False, surface_depth_tol: int = 2,
                 point_surface: str = "splats", landmark_distances: bool = False, distance_pairs=None):
        from ..utils.distances import check_pairs
        from ..utils.render3d import check_point_surface

        # landmark_distances: every prediction leaves a LandmarkDistances (mvlm_amd/utils/distances.py) in ``last_distances``: the
        # straight distance and the distance along the scan's triangles between the landmarks - all pairs, or ``distance_pairs``,
        # a sequence of (i, j).  Measured where the mesh is resident, in the space it was uploaded in, and divided by a pre-align
        # block's scale: the numbers are in the scan's own units.  Off (the default): nothing of it is launched, allocated or copied.
        if not isinstance(landmark_distances, (bool, np.bool_)):
            raise ValueError(f"landmark_distances must be True or False, not {landmark_distances!r}")
        self.landmark_distances = bool(landmark_distances)
        self.distance_pairs = check_pairs(distance_pairs)
        if self.distance_pairs is not None and not self.landmark_distances:
            raise ValueError("distance_pairs needs landmark_distances=True")
        self.last_distances = None

        # point_surface: what a scan without faces - a point cloud - is to every entry that takes scans: "splats" (the default) - it
        # is rendered as splats, snapped to its nearest point, and what needs triangles is refused (_check_cloud); "mesh" - it is
        # replaced by its triangulation (HipRenderer3D.triangulate_point_cloud; DESIGN.md 5.1, "Point clouds") after pre-alignment,
        # and everything downstream sees an ordinary mesh; point_radius and point_normals are then not consulted
        self.point_surface = check_point_surface(point_surface)
        self.render_image_stack = render_image_stack
        self.render_image_folder = render_image_folder
        self.n_views = n_views
        self.visualize_rays = visualize_rays
        self.screenshot_folder = screenshot_folder
        self.device = device
        self.shard_views = shard_views
        self.verbose = verbose
        self.timings: dict[str, float] = {}
        self._timer = StageTimer(self.timings, self._say)
        self.last_error: float | None = None
        # landmark_report: every prediction leaves a LandmarkReport (mvlm_amd/utils/report.py) in ``last_report``: per
        # landmark the surviving views, inliers, RANSAC branch, ray spread, covariance, snap distance and triangle.  Its
        # lengths are in the space the network sees (the pre-aligned model space); only its ``landmarks`` are in file
        # coordinates.  Off (the default): nothing of it is launched, allocated or copied.
        self.landmark_report = bool(landmark_report)
        self.last_report = None
        # the pictures a prediction can leave behind: pictures.py documents every option and checks them
        self.visualize_img = bool(visualize_img)
        self.visualize_size = int(visualize_size)
        self.visualize_rays_img = bool(visualize_rays_img)
        self.visualize_rays_poses = np.asarray(visualize_rays_poses, dtype=np.float64).reshape(-1, 3)
        self.view_png_encoder = check_png_encoder(view_png_encoder)
        self.visualize_sheet = bool(visualize_sheet)
        self.visualize_heat = bool(visualize_heat)
        self.visualize_surface, self.surface_depth_tol = bool(visualize_surface), surface_depth_tol
        self.sheet_scale, self.heat_floor, self.heat_landmarks = sheet_scale, heat_floor, None  # (sheet_scale: of both sheets)
        pictures.check_options(self, n_views, heat_landmarks, visualize_size)
        self.last_view_path = self.last_sheet_path = self.last_heat_path = self.last_surface_path = None
        self.last_surface_heat = self._surface_mesh = None
        self.last_ray_view_paths: list = []
        # the pictures.Pass of the current call, kept only between a prediction made by predict_one_file / predict_files
        # (_keep_ray_view) and the _after_prediction that draws its ray view
        self._ray_view = None
        self._keep_ray_view = False
        name = type(self).__name__.lower()
        self.visualize_name = visualize_name if visualize_name is not None else name[:-len("pipeline")] if name.endswith("pipeline") else name
        self._rays = None  # (mesh, starts, ends) of the current call when visualize_rays is set
        self._buffers: dict = {}
        self._lock = threading.RLock()  # see _serialised
        self._pre_align: dict | None = None
        self.write_pre_aligned_folder: Path | None = None

        retain_freed_host_memory()  # scans come and go: keep their host pages (utils/hostmem.py; MVLM_HOST_MALLOC_TUNING=0 opts out)
        if shard_views:
            # one process per GPU: collectives (RCCL) and the allocator must use THIS rank's device, not cuda:0
            import torch

            if torch.cuda.is_available():
                torch.cuda.set_device(device)
        # render_multisamples: samples per pixel of the renderer (HipRenderer3D.multisamples: 0 or 4)
        # point_radius: splat radius (model units) of scans without faces - point clouds -, None = automatic (HipRenderer3D)
        # point_normals: where a point cloud's normals come from under a geometry image mode: "file" (its own, else refused) or
        # "estimate" (a cloud without gets them estimated on the device) (HipRenderer3D)
        self.renderer_3d = HipRenderer3D(image_size=(256, 256), offscreen=offscreen, n_views=n_views, device=device,
                                         verbose=verbose, multisamples=render_multisamples, point_radius=point_radius,
                                         point_normals=point_normals, point_surface=point_surface)
        self.estimator_3d = HipEstimator3D(device=device, verbose=verbose)
        self.predictor_2d = None  # will be assigned externally

    @property
    def pre_align(self) -> dict | None:
        """Optional "pre-align" block of a Deep-MVLM config (mvlm_amd/utils/prealign.py, utils3d.py:465-527); the
        reference's live pipeline has none (it renders the mesh as-is).  It lives on the renderer slot, which is
        the object that loads meshes; both the fused path and the slot protocol honour it."""
        return getattr(self.renderer_3d, "pre_align", self._pre_align)

    @pre_align.setter
    def pre_align(self, block: dict | None) -> None:
        from ..utils.prealign import is_active

        self._pre_align = block
        if hasattr(self.renderer_3d, "pre_align"):
            self.renderer_3d.pre_align = block
        elif is_active(block):
            raise ValueError("a pre-align block needs a renderer that applies it (HipRenderer3D.pre_align)")

    def _texture_needed(self) -> bool:
        """Does anything downstream read a texture-shaded plane of the views?  The reference always decodes the JPEG
        (utils3d.py:26-36) and renders RGB + depth; a depth or geometry(+depth) model then never looks at the colours.
        Kept: whenever the views are written out (render_image_stack), the scan is drawn (visualize_img) or the views go to a predictor whose planes are unknown."""
        sel = getattr(self.predictor_2d, "chan_sel", None)
        if (self.render_image_stack or self.visualize_img or self.visualize_surface or sel is None
                or not isinstance(self.renderer_3d, HipRenderer3D)):
            return True  # (visualize_img and visualize_surface draw the scan itself: with its texture)
        if self.renderer_3d.shading == "geometry":
            return False  # planes 0..2 carry the build-defined geometry shading
        return any(int(c) < 3 for c in sel)

    def _check_cloud(self, mesh) -> None:
        """A scan without faces - a point cloud - is rendered as splats and snapped to its nearest point; what a cloud does
        not have is said here, before the GPU section, instead of by the call that would meet it."""
        if mesh is None or getattr(mesh, "n_tris", 1) != 0:
            return
        if getattr(self, "point_surface", "splats") == "mesh":
            return  # (the GPU section replaces the cloud by its triangulation, _surface: nothing downstream meets a cloud)
        name = getattr(mesh, "path", None) or "the mesh"
        if self.landmark_report:
            raise ValueError(f"{name} is a point cloud: landmark_report is not supported (the surface attachment needs triangles)")
        if getattr(self, "landmark_distances", False):
            raise ValueError(f"{name} is a point cloud: landmark_distances is not supported (a surface distance needs triangles; "
                             'point_surface="mesh" / --point-surface mesh gives the cloud some)')
        if self.visualize_img:
            raise ValueError(f"{name} is a point cloud: visualize_img is not supported (the landmark view draws triangles)")
        if self.visualize_rays_img:
            raise ValueError(f"{name} is a point cloud: visualize_rays_img is not supported (the ray view draws triangles)")
        if getattr(self, "visualize_surface", False):
            raise ValueError(f"{name} is a point cloud: visualize_surface is not supported (the surface heat colours a mesh's vertices "
                             "and draws its triangles)")
        r3 = self.renderer_3d
        if getattr(r3, "multisamples", 0):
            raise ValueError(f"{name} is a point cloud: multisampled rendering (render_multisamples=4) is not supported")
        # geometry shading needs normals: the cloud's own (a .ply's nx ny nz, a .vtk's NORMALS), or the device's estimate
        if (getattr(r3, "shading", "texture") == "geometry" and getattr(mesh, "normals", None) is None
                and getattr(r3, "point_normals", "file") != "estimate"):
            raise ValueError(f"{name} is a point cloud without normals: a geometry image mode needs them (geometry shading of a point "
                             'cloud: point_normals="estimate" / --point-normals estimate has them estimated)')

    def _surface(self, mesh):
        """``mesh`` itself, or - a point cloud under ``point_surface="mesh"`` - its triangulation (made on the launch stream, so in
        the GPU section and never on a reader thread; kept on the cloud object)."""
        if self.point_surface != "mesh" or mesh is None or getattr(mesh, "n_tris", 1) != 0:
            return mesh
        make = getattr(self.renderer_3d, "triangulate_point_cloud", None)
        if not callable(make):
            raise ValueError('point_surface="mesh" needs a renderer that triangulates a point cloud (HipRenderer3D.triangulate_point_cloud)')
        return make(mesh)

    def _check_distances(self) -> None:
        """``landmark_distances`` needs the renderer that holds the mesh on the device: said before anything is launched."""
        if self.landmark_distances and not isinstance(self.renderer_3d, HipRenderer3D):
            raise ValueError("landmark_distances needs a renderer that measures them (HipRenderer3D.landmark_geodesics), not "
                             f"{type(self.renderer_3d).__name__}")
        if self.landmark_distances and self.distance_pairs is not None and self.predictor_2d is not None:
            from ..utils.distances import check_pairs

            check_pairs(self.distance_pairs, int(self.predictor_2d.get_lm_count()))

    def _measure_distances(self, mesh, landmarks):
        """``landmark_distances``: the distances between ``landmarks`` (in the space of ``mesh``, as the snap left them) on ``mesh``,
        in the scan's own units, into ``last_distances``."""
        found = self.renderer_3d.landmark_geodesics(mesh, np.asarray(landmarks, dtype=np.float64), pairs=self.distance_pairs)
        block = self.pre_align
        scale = float(block.get("scale", 1)) if block and getattr(mesh, "to_original", None) is not None else 1.0
        self.last_distances = found.scaled(scale) if scale != 1.0 else found
        return self.last_distances

    def _to_original(self, mesh, landmarks):
        """Landmarks found on a pre-aligned mesh -> the file's own coordinates (utils3d.py:505-527)."""
        m = getattr(mesh, "to_original", None)
        if m is None or landmarks is None:
            return landmarks
        from ..utils.prealign import landmarks_to_original_space

        return landmarks_to_original_space(landmarks, m)

    def get_lm_count(self) -> int:
        if self.predictor_2d is None:
            raise ValueError("Predictor2D is not initialized.")
        return self.predictor_2d.get_lm_count()

    def _buffer(self, name: str, shape: tuple):
        """A float32 device tensor of this shape that lives as long as the pipeline (one per name)."""
        import torch

        buf = self._buffers.get(name)
        if buf is None or tuple(buf.shape) != tuple(shape):
            buf = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", self.device))
            self._buffers[name] = buf
        return buf

    def _pinned_bytes(self, name: str, n_bytes: int):
        """(pinned uint8 host tensor of exactly this size, its numpy view) that live as long as the pipeline."""
        import torch

        ent = self._buffers.get(name)
        if ent is None or ent[0].numel() != n_bytes:
            t = torch.empty(n_bytes, dtype=torch.uint8).pin_memory()
            ent = self._buffers[name] = (t, t.numpy())
        return ent

    def _buffer_bytes(self, name: str, n_bytes: int):
        """A uint8 device buffer of at least this size that lives as long as the pipeline (8-byte aligned slices)."""
        import torch

        buf = self._buffers.get(name)
        if buf is None or buf.numel() < n_bytes:
            buf = torch.empty((n_bytes + 7) // 8 * 8, dtype=torch.uint8, device=torch.device("cuda", self.device))
            self._buffers[name] = buf
        return buf

    def _say(self, *a):
        if self.verbose:
            print(*a)

    def _fusable(self) -> bool:
        # any predictor that can hand over device-resident maxima for every view (HipPaulsenModel; a
        # PrecomputedPredictor built with ``device_fn``) keeps the whole call in HBM
        p2 = self.predictor_2d
        device_predictor = isinstance(p2, HipPaulsenModel) or callable(getattr(p2, "predict_device", None))
        return (isinstance(self.renderer_3d, HipRenderer3D) and isinstance(self.estimator_3d, HipEstimator3D)
                and device_predictor)

    def predict_one_file(self, file_name: Path, landmark_indices: list[int] | None = None,
                         view_indices: list[int] | None = None, clip_rays_to_mesh: bool = True):
        if self.predictor_2d is None:
            raise ValueError("Predictor2D is not initialized.")
        self._check_visualize()
        file_name = Path(file_name)
        if not file_name.exists():
            print(f"File {file_name} does not exist")
            return None
        # File ingest (OBJ parse, JPEG read - or decode, with texture_decode="host" -: host work, 3-20 ms per scan) and the
        # upload (pinned staging, the library's own copy stream, the JPEG's decode on the device) run BEFORE the pipeline
        # lock is taken: the callers of a server's thread pool (3DMD_server.py:26-31) then ingest their scans side by side
        # and only the GPU section - RNG draws, device buffers, launch graphs, timings - is one caller at a time.
        mesh, load_seconds = None, 0.0
        if self._fusable():
            t0 = time.perf_counter()
            mesh = self._ingest(file_name, self._texture_needed())
            load_seconds = time.perf_counter() - t0
        return self._predict_scan(file_name, mesh, load_seconds, landmark_indices, view_indices, clip_rays_to_mesh)

    def _ingest(self, file_name: Path, load_texture: bool):
        """File -> pre-aligned mesh, checked and uploaded once.  The device copy goes through pinned staging and a copy stream of
        the library's own (mvlm_mesh_upload; the renderer waits for its event), so a reader thread's transfer runs beside the
        current scan's kernels (thread-safe beside a launching thread: include/mvlm_hip.h)."""
        from ..utils.render3d import upload_mesh

        mesh = self.renderer_3d.load_mesh(self.renderer_3d._check_file(file_name), load_texture=load_texture)
        self._check_cloud(mesh)
        upload_mesh(self.renderer_3d.ctx, mesh)
        return mesh

    def _predict_scan(self, file_name, mesh=None, load_seconds=0.0, landmark_indices=None, view_indices=None, clip_rays_to_mesh=True):
        """One scan's GPU section, under the pipeline lock: the per-call ray state, the prediction (fused for a ``mesh`` that is
        ingested and uploaded already, else the slot protocol) under the ``total`` stage, and what follows every prediction.
        ``load_seconds``: what the caller spent on ingest and upload, outside the lock."""
        with self._lock:
            self._rays = None
            self._ray_view, self._keep_ray_view = None, self.visualize_rays_img
            with self._timer.stage("total"):
                landmarks = self._predict_fused(file_name, mesh=mesh) if mesh is not None else self._predict_slots(file_name)
            if mesh is not None:
                self.timings["load"] = self.timings.get("load", 0.0) + load_seconds
                self.timings["total"] += load_seconds
            self._after_prediction(file_name, landmarks, landmark_indices, view_indices, clip_rays_to_mesh)
        return landmarks

    def _after_prediction(self, file_name, landmarks, landmark_indices=None, view_indices=None, clip_rays_to_mesh=True):
        """What follows every prediction, whichever entry point made it (predict_one_file, predict_files):
        the optional ray dump (general_pipeline.py:111-130) and the reset of the per-call ray state."""
        if self.visualize_rays and self._rays is not None:
            try:
                self.dump_rays(file_name, landmarks, landmark_indices, view_indices, clip_rays_to_mesh)
            except Exception as e:  # noqa: BLE001 - general_pipeline.py:129-130: a failed visualisation never fails the call
                print(f"[Pipeline] Ray visualization failed: {e}")
        self._rays = None
        if self.visualize_rays_img and self._ray_view is not None and landmarks is not None:
            try:
                self.draw_ray_view(file_name, landmark_indices, view_indices, clip_rays_to_mesh)
            except Exception as e:  # noqa: BLE001 - as the ray dump: a failed picture never fails the call
                print(f"[Pipeline] Ray view failed: {e}")
        self._ray_view, self._keep_ray_view = None, False

    def draw_ray_view(self, file_name: Path, landmark_indices=None, view_indices=None, clip_to_mesh: bool = True):
        """``visualize_rays_img``: the ray view of the pass kept in ``_ray_view`` (pictures.draw_ray_view)."""
        self._check_visualize()
        return pictures.draw_ray_view(self, self._ray_view, file_name, landmark_indices, view_indices, clip_to_mesh)

    def dump_rays(self, file_name: Path, landmarks, landmark_indices=None, view_indices=None, clip_to_mesh: bool = True):
        """What the reference hands to its VTK ``RayVisualizer`` (general_pipeline.py:111-128), written
        as ``<stem>_rays.npz`` for any viewer: the selected view rays (``starts``, ``ends`` [L,V,3]),
        clipped to their first hit with the mesh when ``clip_to_mesh`` (ray_visualizer.py:172-192,
        here on the GPU: mvlm_clip_rays_to_mesh), ``hit`` [L,V], the indices and the landmarks."""
        mesh, starts, ends = self._rays
        lm_idx, v_idx = select_rays(starts.shape[0], starts.shape[1], landmark_indices, view_indices)
        fs = np.ascontiguousarray(starts[np.ix_(lm_idx, v_idx)])
        fe = np.ascontiguousarray(ends[np.ix_(lm_idx, v_idx)])
        hit = np.zeros(fs.shape[:2], bool)
        if clip_to_mesh and fs.size:
            fe, hit = self.estimator_3d.clip_rays_to_mesh(mesh, fs, fe)
        folder = Path(self.screenshot_folder) if self.screenshot_folder else Path.cwd() / "visualization" / "ray_screenshots"
        folder.mkdir(parents=True, exist_ok=True)
        out = folder / f"{Path(file_name).stem}_rays.npz"
        np.savez(out, starts=fs, ends=fe, hit=hit, landmark_indices=np.asarray(lm_idx), view_indices=np.asarray(v_idx),
                 landmarks=np.asarray(landmarks), clipped=bool(clip_to_mesh))
        self._say(f"[Pipeline] rays written to {out}")
        return out

    # ---- fused device-resident path ----------------------------------------------------
    @_serialised
    def predict_mesh_device(self, mesh, transform_stack):
        """Render + network + fusion + snap for an already loaded mesh and pose table.
        Returns (landmarks [NL,3] float64 numpy, mean RANSAC error).  With
        ``shard_views`` under torch.distributed each rank handles a slice of the views
        (a rank whose slice is empty - more ranks than views - skips render and network
        but still joins the collectives)."""
        import torch

        r3, p2, e3 = self.renderer_3d, self.predictor_2d, self.estimator_3d
        self._check_distances()
        mesh = self._surface(mesh)
        self._check_cloud(mesh)
        drawing = pictures.wanted(self)  # (the one question the hot path asks about the pictures)
        if drawing:
            self._check_visualize()
        n_total = int(transform_stack.shape[0])
        sharded = self.shard_views and parallel.is_distributed()
        rank, world = parallel.rank_world() if sharded else (0, 1)
        lo, hi = parallel.shard_range(n_total, rank, world)

        from ..utils.render3d import view_rotations

        rot = view_rotations(transform_stack)  # once per call: renderer and estimator share it
        tm = self._timer
        dev_t = torch.device("cuda", self.device)
        # this call owns the renderer's / estimator's context until it returns: the launch stream is bound once
        with r3.ctx.hold_stream(torch, dev_t), e3.ctx.hold_stream(torch, dev_t):
            # What the GPU waits for first is the render: single-process, it is enqueued before anything else the host has to
            # prepare (the rotations' second upload, the result buffers, the RANSAC draws: all of that then happens while the
            # rasteriser runs - at 0.5 ms per step, configs[4], the host's serial part is what the step time is made of).
            # Sharded, the draws come out of a collective, which must not queue up behind this step's network: they go first.
            draws_fn = None
            if sharded:
                # one RNG stream for the job: rank 0 draws (global numpy RNG, as the reference) and broadcasts the table
                def draws_fn(counts, keep_on_device=False):
                    draws = e3.draw_ransac_indices(counts) if rank == 0 else None
                    return parallel.broadcast_int32(draws, (len(counts), 8), dev_t, keep_on_device=keep_on_device)

                draws_fn.device_result = True  # plan_draws may ask for the collective's device tensor (RCCL)

            nl_all = p2.get_lm_count()
            plan = e3.plan_draws(nl_all, n_total, draws_fn) if sharded else None
            with tm.stage("render"):
                # one image stack / maxima buffer per view count, reused from call to call: stable addresses let the
                # predictor replay its captured launch graph instead of re-enqueueing ~160 kernels per mesh
                images = None
                if hi > lo:
                    images = r3.render_device(mesh, transform_stack[lo:hi], rot=rot[lo:hi],
                                              out=self._buffer("images", (hi - lo, 256, 256, 4)))
                if self.verbose:
                    torch.cuda.synchronize()
            if images is not None and hi - lo == n_total and r3.ctx is e3.ctx:
                rot_dev = r3.rotations_device()   # all views rendered here: the rays read the rasteriser's own device copy
            else:
                # (enqueued behind the render on the same stream, through pinned staging: the host does not wait)
                rot_dev = e3.upload_rotations_async(rot)
            # landmarks f64[NL,3] | error f64[NL] | survivor counts i32[NL] in ONE buffer: one device-to-host copy per mesh,
            # into pinned memory, enqueued right behind the last kernel
            # (ResultPack); with landmark_report the report rides behind the result in the same buffer: still one copy per mesh.
            # Room for all views: should a detector's ``valid`` mask drop some, the smaller layout made below fits
            rp = ResultPack(nl_all, n_total if self.landmark_report else None)
            pack = self._buffer_bytes("result", rp.total)
            pack_host, pack_np = self._pinned_bytes("result_host", int(pack.numel()))
            dev_views, host, rviews, report = rp.device_views(pack), rp.host_views(pack_np), None, None
            if self.render_image_stack and images is not None:
                self.visualize_image_stack(images.cpu().numpy(), mesh.path or Path("mesh.obj"), first_index=lo)

            kept_views = None  # positions in the pose table of the views a detector's ``valid`` mask left (None: all)
            valid = None  # host bool [views of this rank]: a detector's "nothing found in this view" (None: all valid)
            with tm.stage("prediction"):
                if images is not None and isinstance(p2, HipPaulsenModel):
                    maxima = p2.predict_device(images, out=self._buffer("maxima", (p2.get_lm_count(), hi - lo, 3)))
                elif images is not None:
                    maxima = p2.predict_device(images)
                    if isinstance(maxima, tuple):
                        maxima, valid = maxima
                else:
                    maxima = torch.empty((p2.get_lm_count(), 0, 3), dtype=torch.float32,
                                         device=torch.device("cuda", self.device))
                # (the stack stays where it is until the sheets are drawn)
                sheet_images = images if drawing and pictures.keeps_images(self) else None
                del images
                if sharded:
                    maxima = parallel.all_gather_views(maxima, n_total)
                    if not isinstance(p2, HipPaulsenModel):  # (same predictor class on every rank: all join or none does)
                        valid = parallel.all_gather_valid(valid, hi - lo, n_total, self.device)
                if self.verbose:
                    torch.cuda.synchronize()
            if valid is not None and not valid.all():
                # views without a detection leave the call here, as in the reference (general_pipeline.py:93-95:
                # landmark_stack[:, valid], transform_stack[valid]) - before rays, filter and the RANSAC draws, which
                # address the remaining views by position
                keep = np.nonzero(valid)[0]
                maxima = maxima.index_select(1, torch.from_numpy(keep).to(maxima.device)).contiguous()
                transform_stack = transform_stack[keep]
                rot_dev = e3.upload_rotations_async(rot[keep])
                n_total = int(len(keep))
                kept_views = keep
                if rp.report is not None:
                    rp = ResultPack(nl_all, n_total)
                if plan is not None:  # sharded: the draws planned for all views are void - plan again for the views that remain
                    np.random.set_state(plan["rng_state"])
                    plan = e3.plan_draws(nl_all, n_total, draws_fn)

            if plan is None:
                # the RANSAC draws for the expected survivor counts (~0.3 ms of numpy calls) are made now, while the GPU
                # works on the views; they travel through pinned memory on a copy stream of their own
                plan = e3.plan_draws(nl_all, n_total, None)

            with tm.stage("lines"):
                starts, ends = e3.lines_device(maxima, transform_stack, 256, rot_dev=rot_dev)

            with tm.stage("consensus"):
                if self.visualize_rays:
                    self._rays = (mesh, starts.cpu().numpy(), ends.cpu().numpy())
                if rp.report is not None:
                    rviews = rp.report.device_views(rp.report_bytes(pack))
                    rviews["scores"].copy_(maxima[:, :, 2])
                # (with a report, every solve - the one verify may repeat too - is followed by the report kernel)
                out, err, verify = e3.consensus_device(maxima, starts, ends, deferred=True, plan=plan, err_out=dev_views["error"],
                                                       count_out=dev_views["counts"], report=rviews)

            def snap():
                e3.project_device(mesh, out, out=dev_views["snapped"])
                if rviews is not None:  # behind the snap: the same search once more, leaving triangle, weights and uv
                    e3.attach_device(mesh, out, views=rviews)

            with tm.stage("project"):
                # the snap is enqueued before anything is fetched: one wait and one copy per mesh, at the end
                snap()
                stream = torch.cuda.current_stream(dev_t)
                pack_host.copy_(pack, non_blocking=True)
                stream.synchronize()
                if verify(counts=host["counts"]):
                    # the RANSAC draws had to be repeated for other survivor counts (tied / NaN scores, absolute mode)
                    snap()
                    pack_host.copy_(pack, non_blocking=True)
                    stream.synchronize()
                landmarks = host["snapped"].copy()  # (the pinned staging buffer is the next call's too)
                error = e3.mean_error(host["error"])
                r3.check()  # deferred renderer status (the stream has been waited for above)
                if rp.report is not None:
                    # (model space; _predict_fused maps ``landmarks`` back to the file's coordinates.  Should the fp16 range guard
                    # below repeat the scan, the repeated pass leaves its own report here.)
                    report = self.last_report = LandmarkReport(rp.report.host_arrays(rp.report_bytes(pack_np)), landmarks=landmarks,
                                                               view_indices=kept_views)
            asked16 = getattr(p2, "configured_precision", getattr(p2, "precision", None)) == "fast16"
            if asked16:
                # an activation beyond fp16's range somewhere in the network (the kernel raised the context's flag; the maxima of
                # the pass carry NaN scores, which survive no filter - the landmarks above are finite nonsense).  Same scan again
                # on bf16x3; asked here, after the step's own wait for its results, the question costs one 4-byte copy.
                # (the global RNG stands behind this call's draws: the repeat draws again, as a second call would.)
                # Sharded: the decision is taken by all ranks together - a rank repeating alone would wait in collectives nobody
                # else joins - and WHETHER to ask is decided from what the caller configured, which is the same on every rank:
                # a rank that already fell back on its own (predict_landmarks_from_images) still joins the all-reduce.
                mine = p2.precision == "fast16" and p2.fast16_overflowed()
                if parallel.any_rank(mine, self.device) if sharded else mine:
                    return p2.repeat_without_fp16(lambda: self.predict_mesh_device(mesh, transform_stack))
            self._say("Landmarks [Error]: ", f"{error:08.6f}", " mm")
            self.last_error = error
            if self.landmark_distances and (not sharded or rank == 0):  # (sharded: every rank holds the landmarks, one measures)
                with tm.stage("distances"):
                    self._measure_distances(mesh, landmarks)
            if drawing:
                if kept_views is not None and sheet_images is not None:  # the views a detector's ``valid`` mask left
                    sheet_images = sheet_images.index_select(0, torch.from_numpy(np.asarray(kept_views)).to(sheet_images.device))
                    rot = rot[kept_views]
                # (sharded: every rank holds the result, one draws)
                pictures.draw(self, pictures.Pass(mesh, sheet_images, maxima, rot, starts, ends, landmarks, report, not sharded or rank == 0))
            return landmarks, error

    def _check_visualize(self):
        """What the picture flags need of the slots and the run (pictures.check): said before the prediction, not after it."""
        pictures.check(self)

    def _draw_landmark_view(self, mesh, landmarks, report=None):
        """``visualize_img`` (pictures.draw_landmark_view); ``report``: the LandmarkReport of THIS prediction or None."""
        return pictures.draw_landmark_view(self, mesh, landmarks, report)

    def write_surface_mesh(self, path):
        """``visualize_surface``: the last scan's mesh with the surface heat's colours per vertex, as an OBJ (pictures.write_surface_mesh)."""
        return pictures.write_surface_mesh(self, path)

    def _groupable(self, n_scans: int) -> bool:
        """Can ``n_scans`` scans share one network pass (predict_meshes_device)?"""
        p2, e3 = self.predictor_2d, self.estimator_3d
        if n_scans < 2 or not self._fusable() or not isinstance(p2, HipPaulsenModel):
            return False
        if p2.precision == "fast16":
            return False  # the fp16 range guard (and its fallback) works scan by scan
        if (self.shard_views and parallel.is_distributed()) or self.render_image_stack or self.visualize_rays:
            return False
        if self.landmark_report:
            return False  # one report per scan, made by the scan's own pass
        if self.landmark_distances:
            return False  # likewise the distances: measured while the scan's mesh is resident
        if self.visualize_img or self.visualize_rays_img or self.visualize_sheet or self.visualize_heat or self.visualize_surface:
            return False  # one picture per scan, drawn by the scan's own pass while its mesh (its views) are resident
        n = int(self.renderer_3d.n_views)
        return e3.expected_counts(p2.get_lm_count(), n) is not None and n_scans * n <= (p2.device_batch or 128)

    @_serialised
    def predict_meshes_device(self, meshes, pose_fn=None):
        """Several loaded scans through ONE pass of the network: with few views per scan (the reference's default 8) a
        pass over 8 views runs the matrix cores at 0.64 of what a pass over 64 does.  Every scan is rendered into its
        slice of one image stack, the network runs once, rays / consensus / snap follow per scan and ONE copy brings all
        results back.  The global RNG is consumed exactly as by a loop of ``predict_mesh_device``: poses of scan 1, draws
        of scan 1, poses of scan 2, ... - the draws being the speculative ones of ``plan_draws``; if a scan's survivor
        counts differ from the expectation (tied / NaN scores), that scan's draws are repeated from the saved RNG
        state and the scans after it are processed one by one from there.  Returns [(landmarks, error), ...]; falls back
        to the loop when the scans cannot share a pass (``_groupable``).  With ``landmark_report`` the scans always go one
        by one and ``last_report`` is the LAST scan's when this returns: a caller that wants every scan's report uses
        ``predict_files`` (one report per yielded scan) or calls ``predict_mesh_device`` per mesh."""
        import torch

        from ..utils.render3d import view_rotations

        r3, p2, e3 = self.renderer_3d, self.predictor_2d, self.estimator_3d
        pose_fn = pose_fn or r3.generate_3d_transformations
        k = len(meshes)
        from ..utils.prealign import aligned

        meshes = [self._surface(aligned(m, self.pre_align)) for m in meshes]
        # (a point cloud among them: the scans go one by one - grouping clouds is not built)
        if not self._groupable(k) or any(m.n_tris == 0 for m in meshes):
            out = []
            for m in meshes:
                landmarks, err = self.predict_mesh_device(m, pose_fn())
                out.append((self._report_landmarks(self._to_original(m, landmarks)), err))
            return out
        nl, n = p2.get_lm_count(), int(r3.n_views)
        rp = ResultPack(nl)
        per = rp.nbytes  # a scan's stride in the shared buffer
        stacks, rots, rot_devs, plans = [], [], [], []
        for j in range(k):  # the host's RNG work first, in the loop's order; uploads while the stream is empty
            ts = pose_fn()
            if int(ts.shape[0]) != n:
                raise ValueError("predict_meshes_device: every scan needs the pipeline's n_views poses")
            rot = view_rotations(ts)
            stacks.append(ts)
            rots.append(rot)
            plans.append(e3.plan_draws(nl, n, None, slot=j))
            rot_devs.append(e3.upload_rotations(rot))
        tm = self._timer
        with tm.stage("render"):
            images = self._buffer("images_group", (k * n, 256, 256, 4))
            for j in range(k):
                r3.render_device(meshes[j], stacks[j], rot=rots[j], out=images[j * n:(j + 1) * n])
        with tm.stage("prediction"):
            maxima = p2.predict_device(images, out=self._buffer("maxima_group", (nl, k * n, 3)))
        pack = self._buffer_bytes("result_group", k * per)
        pending = []
        with tm.stage("consensus"):
            for j in range(k):
                views = rp.device_views(pack[j * per:(j + 1) * per])
                mj = maxima[:, j * n:(j + 1) * n].contiguous()
                starts, ends = e3.lines_device(mj, stacks[j], 256, rot_dev=rot_devs[j])
                out, _, verify = e3.consensus_device(mj, starts, ends, deferred=True, plan=plans[j], err_out=views["error"],
                                                     count_out=views["counts"])
                e3.project_device(meshes[j], out, out=views["snapped"])
                pending.append((out, verify, views["snapped"]))
        results = []

        def unpack(host_seg):
            fetched = rp.host_views(host_seg)
            return fetched["snapped"].copy(), e3.mean_error(fetched["error"])

        def original(j, res):
            return self._to_original(meshes[j], res[0]), res[1]

        with tm.stage("project"):
            host = pack[: k * per].cpu().numpy()
            for j in range(k):
                out, verify, snap_view = pending[j]
                seg = host[j * per:(j + 1) * per]
                if verify(counts=rp.host_views(seg)["counts"]):
                    # other survivor counts than planned: this scan's draws + solve were repeated from its saved RNG
                    # state; the RNG now stands where the loop would have it, so the remaining scans go one by one
                    e3.project_device(meshes[j], out, out=snap_view)
                    results.append(original(j, unpack(pack[j * per:(j + 1) * per].cpu().numpy())))
                    for i in range(j + 1, k):
                        results.append(original(i, self.predict_mesh_device(meshes[i], pose_fn())))
                    break
                results.append(original(j, unpack(seg)))
            r3.check()
        self.last_error = results[-1][1]
        return results

    def predict_files(self, files, prefetch: int = 2, readers: int | None = None, batch_scans: int = 1):
        """``predict_one_file`` over many scans, yielding ``(file, landmarks | None)`` in order.

        The reference's CLI loops ``predict_one_file`` (main.py:55-62), paying file ingest and GPU
        work back to back.  Here a reader thread parses the next ``prefetch`` OBJ/JPEG pairs
        (native reader + libjpeg, both outside the GIL) while the GPU works on the current scan,
        so a folder runs at the GPU rate.  With few views per scan (the reference's default 8) one
        reader is slower than the GPU: ``readers`` threads (default: a quarter of the host's cores,
        1..4) parse ``max(prefetch, readers + 1)`` scans ahead; delivery stays in file order.  Results
        equal the sequential loop's: poses and RANSAC draws are taken on the calling thread in file
        order, and every scan gets the same post-step (ray dump) as ``predict_one_file``.
        ``batch_scans`` > 1: that many consecutive scans share one pass of the network
        (``predict_meshes_device``; same results, higher throughput when a scan has few views)."""
        from concurrent.futures import ThreadPoolExecutor

        files = [Path(f) for f in files]
        if self.predictor_2d is None:
            raise ValueError("Predictor2D is not initialized.")
        self._check_visualize()
        if not self._fusable() or prefetch <= 0:
            for f in files:
                yield f, self.predict_one_file(f)
            return

        load_texture = self._texture_needed()

        def ingest(f: Path):  # (on a reader thread)
            return self._ingest(f, load_texture) if f.exists() else None

        if readers is None:
            readers = min(4, max(1, (os.cpu_count() or 4) // 4))
        readers = max(1, int(readers))
        batch_scans = max(1, int(batch_scans))
        if batch_scans > 1 and not self._groupable(batch_scans):
            batch_scans = 1
        prefetch = max(int(prefetch), readers + 1, 2 * batch_scans if batch_scans > 1 else 0)
        with ThreadPoolExecutor(max_workers=readers, thread_name_prefix="mvlm-ingest") as pool:
            pending = [pool.submit(ingest, f) for f in files[:prefetch]]
            group: list = []  # (file, mesh) of scans waiting to share a network pass

            def flush():
                if not group:
                    return
                with self._lock:  # held for the group's GPU section only, never across a yield
                    with self._timer.stage("total"):
                        results = self.predict_meshes_device([m for _, m in group])
                    for (gf, gm), (landmarks, _) in zip(group, results):
                        self._dump_pre_aligned(gm, gf)  # (ingest pre-aligned the scan)
                        self._after_prediction(gf, landmarks)
                done = [(gf, landmarks) for (gf, _), (landmarks, _) in zip(group, results)]
                pool.submit(_drop, [m for _, m in group])
                group.clear()
                yield from done

            for i, f in enumerate(files):
                if i + prefetch < len(files):
                    pending.append(pool.submit(ingest, files[i + prefetch]))
                try:
                    mesh = pending.pop(0).result()  # re-raises the reader's ValueError / FileNotFoundError
                except BaseException:
                    # the one-by-one loop would have delivered every scan before the malformed one: the scans
                    # waiting in the group get their results first, then the error goes to the caller
                    yield from flush()
                    raise
                if mesh is None:
                    yield from flush()
                    print(f"File {f} does not exist")
                    yield f, None
                    continue
                if batch_scans > 1:
                    group.append((f, mesh))
                    del mesh
                    if len(group) == batch_scans or i + 1 == len(files):
                        yield from flush()
                    continue
                landmarks = self._predict_scan(f, mesh)
                # returning a scan's 10-25 MB of host arrays to the OS costs milliseconds (page
                # unmapping under the GPU driver's MMU notifier): let the reader thread drop them
                # while this thread goes on to the next scan
                pool.submit(_drop, [mesh])
                del mesh
                yield f, landmarks
            yield from flush()

    def _predict_fused(self, file_name: Path, mesh=None):
        from ..utils.prealign import aligned

        t0 = time.perf_counter()
        if mesh is None:
            file_name = self.renderer_3d._check_file(file_name)
            mesh = self.renderer_3d.load_mesh(file_name, load_texture=self._texture_needed())
        else:
            mesh = aligned(mesh, self.pre_align)
        mesh = self._surface(mesh)
        sharded = self.shard_views and parallel.is_distributed()
        if sharded:
            rank, _ = parallel.rank_world()
            poses = self.renderer_3d.generate_3d_transformations() if rank == 0 else None
            poses = parallel.broadcast_array(poses, (int(self.renderer_3d.n_views), 6), device=self.device)
        else:
            poses = self.renderer_3d.generate_3d_transformations()
        self.timings["load"] = time.perf_counter() - t0
        self._dump_pre_aligned(mesh, file_name)
        landmarks, _ = self.predict_mesh_device(mesh, poses)
        return self._report_landmarks(self._to_original(mesh, landmarks))

    def _report_landmarks(self, landmarks):
        """The last report's ``landmarks`` are what the caller gets: the file's coordinates."""
        if self.landmark_report and self.last_report is not None and landmarks is not None:
            self.last_report.landmarks = np.array(landmarks, dtype=np.float64)
        return landmarks

    def _dump_pre_aligned(self, mesh, file_name):
        """``pre-align.write_pre_aligned`` (utils3d.py:489-494): the transformed surface as a legacy .vtk file."""
        block = self.pre_align
        if not (block and block.get("write_pre_aligned") and getattr(mesh, "to_original", None) is not None):
            return
        from ..utils.prealign import write_pre_aligned

        folder = Path(self.write_pre_aligned_folder) if self.write_pre_aligned_folder else Path(file_name).parent
        write_pre_aligned(mesh, folder / f"{Path(file_name).stem}_pre_transform_mesh.vtk")

    # ---- the reference's numpy slot protocol (general_pipeline.py:83-108) ----------------
    def _predict_slots(self, file_name: Path):
        tm = self._timer
        self._check_distances()
        with tm.stage("render"):
            if isinstance(self.renderer_3d, HipRenderer3D):
                image_stack, transform_stack, pd = self.renderer_3d.multiview_render(file_name, load_texture=self._texture_needed())
            else:
                image_stack, transform_stack, pd = self.renderer_3d.multiview_render(file_name)
        self._check_cloud(pd)
        if self.render_image_stack:
            self.visualize_image_stack(image_stack, file_name)
        with tm.stage("prediction"):
            landmark_stack, valid = self.predictor_2d.predict_landmarks_from_images(image_stack)
        landmark_stack = landmark_stack[:, valid, :]
        transform_stack = transform_stack[valid]
        image_stack = image_stack[valid]
        with tm.stage("lines"):
            lines_s, lines_e = self.estimator_3d.estimate_landmark_lines(image_stack, landmark_stack, transform_stack)
        if self.visualize_rays:
            self._rays = (pd, np.asarray(lines_s), np.asarray(lines_e))
        arrays = None
        if self.landmark_report and not (callable(getattr(self.estimator_3d, "estimate_landmarks_from_lines_report", None))
                                         and callable(getattr(self.estimator_3d, "attach_landmarks_to_surface", None))):
            raise ValueError("landmark_report needs an estimator with estimate_landmarks_from_lines_report and "
                             "attach_landmarks_to_surface (HipEstimator3D)")
        with tm.stage("consensus"):
            if self.landmark_report:
                landmarks, error, arrays = self.estimator_3d.estimate_landmarks_from_lines_report(landmark_stack, lines_s, lines_e)
            else:
                landmarks, error = self.estimator_3d.estimate_landmarks_from_lines(landmark_stack, lines_s, lines_e)
        with tm.stage("project"):
            if arrays is not None:
                arrays.update(self.estimator_3d.attach_landmarks_to_surface(pd, landmarks))
                landmarks = arrays["snapped"]
            else:
                landmarks = self.estimator_3d.project_landmarks_to_surface(pd, landmarks)
        self._say("Landmarks [Error]: ", f"{error:08.6f}", " mm")
        self.last_error = error
        self._dump_pre_aligned(pd, file_name)
        drawn = landmarks  # (the picture: in the space the mesh was rendered in)
        if self.landmark_distances:
            with tm.stage("distances"):
                self._measure_distances(pd, drawn)
        # a mesh handle that went through the config's pre-align block carries its matrix: results go back to
        # the file's coordinates (the rays kept for visualisation stay in the aligned space, with the mesh handle)
        landmarks = self._to_original(pd, landmarks)
        report = None
        if arrays is not None:
            kept = np.asarray(valid)
            report = self.last_report = LandmarkReport(arrays, landmarks=landmarks,
                                              view_indices=np.nonzero(kept)[0] if kept.dtype == bool else kept)
        if pictures.wanted(self):  # behind the report: the pictures carry THIS scan's branches
            from ..utils.render3d import view_rotations

            pictures.draw(self, pictures.Pass(pd, np.asarray(image_stack, dtype=np.float32), np.asarray(landmark_stack, dtype=np.float32),
                                              view_rotations(np.asarray(transform_stack)), np.asarray(lines_s), np.asarray(lines_e),
                                              drawn, report))
        return landmarks

    def visualize_image_stack(self, image_stack: np.ndarray, file_name: Path, first_index: int = 0):
        """PNG dump of the rendered views (general_pipeline.py:133-146)."""
        from PIL import Image

        save_folder = self.render_image_folder or Path(file_name).parent
        if not Path(save_folder).exists():
            raise ValueError(f"Folder for --visualize-method flag [{save_folder}] does not exist.")
        for i in range(image_stack.shape[0]):
            single_image = np.uint8(image_stack[i, :, :, 0:3] * 255)
            Image.fromarray(single_image).save(Path(save_folder) / f"{Path(file_name).stem}_{first_index + i:02d}.png")
