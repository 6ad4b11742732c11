"""Command line front end: ``python -m mvlm_amd -p <obj or folder> [-o out] [-n views]``.

Same behaviour as the reference's ``main.py`` (:9-67): collect ``*.obj`` files, run every
available pipeline over them and write ``<stem>_<pipeline>.txt`` (comma-separated [NL,3]
landmarks, ``np.savetxt(..., delimiter=",")``, main.py:62; with ``--report`` also ``<stem>_<pipeline>_report.csv``, the
per-landmark quality report of mvlm_amd/utils/report.py; with ``--distances`` also ``<stem>_<pipeline>_distances.csv``, the
straight and surface distances between the landmarks, mvlm_amd/utils/distances.py).  Only the pipelines whose 2-D
predictor this build ships are looped ("bu3dfe", "dtu3d").  ``--visualize-img`` (main.py:66-67) writes
``visualization/<stem>_<pipeline>.png`` under the working directory: the scan with a sphere at every landmark, drawn on the GPU
(mvlm_amd/utils/viewer.py); the interactive viewer flag of the reference (``--visualize-iter``) needs VTK and is not available.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

import numpy as np


def shard_files(files, rank: int, world: int):
    """Round-robin share of ``files`` for ``rank`` of ``world`` processes (order preserved)."""
    return [f for i, f in enumerate(files) if i % world == rank]


def _index_list(text: str) -> list:
    """"3,17,40" -> [3, 17, 40] (argparse reports what is no such list)."""
    return [int(k) for k in text.split(",")]


def _pairs(text: str):
    """"0-16,8-27" -> [(0, 16), (8, 27)] (argparse reports what is no such list)."""
    from .utils.distances import parse_pairs

    try:
        return parse_pairs(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog="python -m mvlm_amd")
    parser.add_argument("-p", "--path", type=str, required=True)
    parser.add_argument("-o", "--out", type=str, required=False)
    parser.add_argument("-n", "--n-views", type=int, default=None, help="Number of views to render (default: 8, or the config's)")
    parser.add_argument("--visualize-method", action="store_true", help="Dump the rendered views as PNG next to the mesh")
    parser.add_argument("--pipelines", type=str, default="bu3dfe,dtu3d")
    parser.add_argument("-c", "--config", type=str, default=None,
                        help="a Deep-MVLM JSON config (path, or the stem of one of the reference's configs/*.json, e.g. "
                             "BU_3DFE-depth): ONE pipeline built from its inference keys - model, image channels, view count "
                             "(unless -n is given), pose ranges, line filter, pre-align block - instead of --pipelines")
    parser.add_argument("--weights", type=str, default=None,
                        help='checkpoint path, or "synthetic[:seed]" (no checkpoint is reachable offline)')
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--precision", choices=("exact", "fast", "fast16"), default="exact",
                        help="exact: fp32 on the matrix cores (default, the parity path); fast: the big 3x3 layers on "
                             "bf16x3-split operands (fp32-accurate, not bit-identical; DESIGN.md 4.1b)")
    parser.add_argument("--batch-scans", type=int, default=1,
                        help="that many consecutive scans share one pass of the network (higher throughput at few views per "
                             "scan; a near-tied heatmap maximum may resolve differently than in the one-by-one loop)")
    parser.add_argument("--seed", type=int, default=None,
                        help="seed of the global numpy RNG (poses for N != 8 views and the RANSAC draws come from it, as in the "
                             "reference, which never seeds it): makes a run reproducible")
    parser.add_argument("--multisamples", type=int, choices=(0, 4), default=0,
                        help="samples per pixel of the renderer: 0 = one at the pixel centre (default), 4 = multisampled views "
                             "(for checkpoints trained on multisampled VTK renders; DESIGN.md 5.1)")
    parser.add_argument("--report", action="store_true",
                        help="write <stem>_<pipeline>_report.csv beside every landmark file: one row per landmark with the surviving "
                             "views, inliers, RANSAC branch, ray spread, snap distance, triangle, barycentric weights and uv "
                             "(lengths in the space the network sees; x,y,z in file coordinates; INTEGRATION.md)")
    parser.add_argument("--visualize-img", action="store_true",
                        help="write visualization/<stem>_<pipeline>.png under the working directory for every scan: the mesh with a "
                             "sphere at every landmark (with --report the spheres are coloured by the RANSAC branch: blue inlier fit, "
                             "orange fallback to all lines, red fewer than three lines)")
    parser.add_argument("--visualize-size", type=int, default=1024,
                        help="side of that picture, and of --visualize-rays' pictures, in pixels (a multiple of 16, 64..2048)")
    parser.add_argument("--visualize-rays", action="store_true",
                        help="write visualization/ray_screenshots/<stem>_<pipeline>_rays_<i>.png under the working directory for every "
                             "scan: the mesh, every view's ray for every landmark clipped to its first hit with the surface, and the "
                             "landmarks, from the front and from 60 degrees left and right (with --report the rays are green where the "
                             "consensus used them, orange where it kept but did not use them, grey where the score filter dropped them)")
    parser.add_argument("--visualize-sheet", action="store_true",
                        help="write visualization/<stem>_<pipeline>_views.png under the working directory for every scan: all rendered "
                             "views in one picture, a marker where the network put each landmark in each view and a red line from it "
                             "to where the final landmark projects in that view (with --report a view the score filter dropped gets a "
                             "ring, and the markers carry the RANSAC branch colours)")
    parser.add_argument("--sheet-scale", type=int, default=1, choices=(1, 2, 3, 4),
                        help="sheet pixels per view pixel of --visualize-sheet and --visualize-heat (the sheet may not exceed 4096 pixels "
                             "a side)")
    parser.add_argument("--visualize-heat", action="store_true",
                        help="write visualization/<stem>_<pipeline>_heat.png under the working directory for every scan: all rendered "
                             "views in one picture with the network's heatmaps laid over them, per pixel the landmark whose value is the "
                             "largest share of its heatmap's peak, in that landmark's colour (costs about one network pass more per scan)")
    parser.add_argument("--heat-landmarks", type=_index_list, default=None, metavar="L,L,...",
                        help="the landmarks --visualize-heat shows, e.g. 3,17,40 (default: all)")
    parser.add_argument("--heat-floor", type=float, default=0.25, metavar="F",
                        help="--visualize-heat draws a heatmap only where it exceeds this share of its peak (0 <= F < 1)")
    parser.add_argument("--visualize-surface", action="store_true",
                        help="write visualization/<stem>_<pipeline>_surface.png under the working directory for every scan: the mesh "
                             "with all views' heatmaps laid on it, per vertex the landmark with the largest mean share of its heatmaps' "
                             "peaks over the views that see the vertex, and the final landmarks as spheres (--heat-landmarks and "
                             "--heat-floor apply; costs about one network pass more per scan, shared with --visualize-heat)")
    parser.add_argument("--surface-depth-tol", type=int, default=2, metavar="STEPS",
                        help="--visualize-surface: depth steps (1/255 of the clip range, 5.9 model units) a vertex may lie behind a "
                             "view's rendered surface and still count as seen there (0..255)")
    parser.add_argument("--surface-mesh", action="store_true",
                        help="with --visualize-surface (which it turns on): also write <stem>_<pipeline>_surface.obj beside the "
                             "landmark file, the scan with those colours per vertex")
    parser.add_argument("--point-radius", type=float, default=None, metavar="MM",
                        help="splat radius, in model units, of scans that have points but no faces (point clouds): 0.88 to 9.375, "
                             "i.e. 0.75 to 8 pixels of a view; default: automatic, from the spacing of the points (DESIGN.md 5.1)")
    parser.add_argument("--point-normals", choices=("file", "estimate"), default="file",
                        help="where a point cloud's normals come from under a geometry image mode: 'file' takes the scan's own (a "
                             "cloud without is refused), 'estimate' has the GPU estimate them from each point's 16 nearest neighbours "
                             "(DESIGN.md 5.1)")
    parser.add_argument("--point-surface", choices=("splats", "mesh"), default="splats",
                        help="what a scan without faces (a point cloud) is to the pipeline: 'splats' renders it as splats, snaps "
                             "to its nearest point and refuses what needs triangles (--report, --visualize-img, --visualize-rays, "
                             "--visualize-surface, --multisamples 4); 'mesh' has the GPU give it triangles first - a local Delaunay "
                             "surface over each point's 16 nearest neighbours, for scanner-like sampling - and then treats it as any "
                             "mesh; --point-radius and --point-normals are then not consulted (DESIGN.md 5.1)")
    parser.add_argument("--distances", action="store_true",
                        help="write <stem>_<pipeline>_distances.csv beside every landmark file: one row per pair of landmarks i < j with "
                             "the straight distance and the distance along the scan's surface (geodesic: the mean of the two directions "
                             "geodesic_ij and geodesic_ji, whose difference says how far to trust it), in the scan's own units; inf: the "
                             "landmarks lie on separate pieces of the scan.  The surface distance is a first-order fast-marching "
                             "estimate, a few per cent above the true one (DESIGN.md 5.1); a point cloud needs --point-surface mesh")
    parser.add_argument("--distance-pairs", type=_pairs, default=None, metavar="I-J,I-J",
                        help="with --distances: only these pairs of landmark indices, e.g. 0-16,8-27 (default: every pair)")
    parser.add_argument("--png-encoder", choices=("host", "device"), default="host",
                        help="who makes the PNG files of --visualize-img and --visualize-rays: 'host' copies the picture to the host "
                             "and encodes it with Pillow; 'device' filters and compresses it on the GPU and copies only the file's "
                             "bytes (the same pixels, other bytes)")
    return parser


def main(argv=None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.out is None:
        args.out = args.path
    input_path, path_to_out = Path(args.path), Path(args.out)
    if not input_path.exists():
        print(f"{input_path.as_posix()} does not exist.")
        return 1
    if input_path.is_file():
        if input_path.suffix.lower() != ".obj":
            print(f"{input_path.as_posix()} is not an .obj file.")
            return 1
        obj_files = [input_path]
        if args.out == args.path:
            path_to_out = input_path.parent
    else:
        obj_files = sorted(input_path.glob("*.obj"))
        if len(obj_files) == 0:
            print("Given folder does not contain any .obj files.")
            return 1
    path_to_out.mkdir(parents=True, exist_ok=True)
    # one process per GPU (python -m torch.distributed.run --nproc-per-node N -m mvlm_amd -p folder/): scans are
    # independent, so rank r simply takes every N-th file on its own GPU - no collective, N times the folder rate
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        obj_files = shard_files(obj_files, rank, world)
        if args.device == 0:
            args.device = int(os.environ.get("LOCAL_RANK", "0"))
        print(f"[rank {rank}/{world}] {len(obj_files)} scans on GPU {args.device}")

    from . import pipeline

    extra = {"precision": args.precision} if args.precision != "exact" else {}
    if args.multisamples:
        extra["render_multisamples"] = args.multisamples
    if args.report:
        extra["landmark_report"] = True
    if args.visualize_img:
        extra["visualize_img"] = True
        extra["visualize_size"] = args.visualize_size
    if args.visualize_rays:
        extra["visualize_rays_img"] = True
        extra["visualize_size"] = args.visualize_size
    if args.visualize_sheet:
        extra["visualize_sheet"] = True
        extra["sheet_scale"] = args.sheet_scale
    if args.visualize_heat:
        extra["visualize_heat"] = True
        extra["sheet_scale"] = args.sheet_scale
        extra["heat_landmarks"] = args.heat_landmarks
        extra["heat_floor"] = args.heat_floor
    if args.visualize_surface or args.surface_mesh:
        extra["visualize_surface"] = True
        extra["visualize_size"] = args.visualize_size
        extra["surface_depth_tol"] = args.surface_depth_tol
        extra["heat_landmarks"] = args.heat_landmarks
        extra["heat_floor"] = args.heat_floor
    if args.distance_pairs is not None and not args.distances:
        parser.error("--distance-pairs needs --distances")
    if args.distances:
        extra["landmark_distances"] = True
        extra["distance_pairs"] = args.distance_pairs
    if args.point_radius is not None:
        extra["point_radius"] = args.point_radius
    if args.point_normals != "file":
        extra["point_normals"] = args.point_normals
    if args.point_surface != "splats":
        extra["point_surface"] = args.point_surface
    if args.png_encoder != "host":
        extra["view_png_encoder"] = args.png_encoder
    if args.config is not None:
        from . import config as mvlm_config

        src = args.config if Path(args.config).is_file() else mvlm_config.default_config(args.config)
        jobs = [(Path(args.config).stem, lambda: pipeline.pipeline_from_config(
            src, n_views=args.n_views, weights=args.weights, device=args.device,
            **({"render_image_stack": True} if args.visualize_method else {}), **extra))]
    else:
        jobs = [(p, (lambda p=p: pipeline.create_pipeline(p, render_image_stack=args.visualize_method, n_views=args.n_views or 8,
                                                          weights=args.weights, device=args.device, **extra)))
                for p in args.pipelines.split(",") if p]
    for pname, make in jobs:
        print(f"Pipeline: {pname}")
        if args.seed is not None:
            np.random.seed(args.seed)
        dm = make()
        dm.visualize_name = pname
        # ingest of the next scans overlaps the GPU work
        for file, landmarks in dm.predict_files(obj_files, batch_scans=args.batch_scans):
            print(f"Current file: {file}")
            if landmarks is None:
                print(f"Landmarks for {file} could not be predicted -> skipping file [{file.stem}] for pipeline {pname}")
                continue
            np.savetxt((path_to_out / f"{file.stem}_{pname}.txt").as_posix(), landmarks, delimiter=",")
            if args.report:
                dm.last_report.to_csv(path_to_out / f"{file.stem}_{pname}_report.csv")
            if args.distances:
                dm.last_distances.to_csv(path_to_out / f"{file.stem}_{pname}_distances.csv")
            if args.surface_mesh:
                dm.write_surface_mesh(path_to_out / f"{file.stem}_{pname}_surface.obj")
    return 0


if __name__ == "__main__":
    sys.exit(main())
