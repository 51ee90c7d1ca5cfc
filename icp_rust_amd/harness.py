"""Headless frame loops of the reference's two examples: same file
handling, same warm start, same per-frame `Icp::new` + `estimate(src, transform, 20)`, the
trajectory instead of a window.

`icp_factory(dst) -> object with .estimate(src, Transform, max_iter) -> Transform` defaults to
the GPU classes; tests inject an oracle-backed factory to check the loop semantics on CPU.
"""
import os

import numpy as np

from .api import Icp2d, Icp3d, Transform, remove_statistical_outliers, voxel_centroids, voxel_downsample
from .scans import PacketFile, load_scan2d, write_packets
from .synth import PACKETS_PER_FRAME, remove_invalid_values


def run_scan2d(scan_dir, max_iter=20, icp_factory=None, max_frames=None, point_to_line=None, qualities=None,
               quality_distance=None):
    """examples/scan2d.rs:62-115.  `index` starts at 0 and is incremented BEFORE use, so
    000.txt is never read and 001.txt is the fixed source (:63,69-77); every later frame k
    loads dst = k.txt, builds Icp2d::new(&dst) and estimates warm-started from the previous
    frame (:85-88); the plotted pose is transform.inverse() (:90) and its translation is
    appended to the path (:105).  The loop ends at the first missing file (:72).
    `point_to_line=k` (EXTENSION, not in the reference; include/icp_mi355x.h section 14): every frame's handle computes
    the line normals of its targets from their k nearest (compute_line_normals(k)) and registers with the point-to-line
    residual (estimate_point_to_line) instead; None calls exactly what it always called.
    `qualities=[]` (EXTENSION; sections 9 and 16): after each frame's estimate the list gets the score of the estimated
    pose on that frame's handle, within quality_distance (None: +inf) -- evaluate_point_to_line (a LineQuality) when
    point_to_line is set, evaluate (a Quality) otherwise; None calls neither.
    Returns (transforms, inverse_transforms, path_xy)."""
    icp_factory = icp_factory or Icp2d
    index = 0
    src = None
    transform = Transform.identity()
    transforms, inverses, path = [], [], []
    while max_frames is None or len(transforms) < max_frames:
        index += 1
        filename = os.path.join(scan_dir, f"{index:03d}.txt")
        if not os.path.exists(filename):
            break
        if index == 1:
            src = load_scan2d(filename)
            continue
        dst = load_scan2d(filename)
        icp = icp_factory(dst)
        if point_to_line:
            icp.compute_line_normals(point_to_line)
            transform = icp.estimate_point_to_line(src, transform, max_iter)
        else:
            transform = icp.estimate(src, transform, max_iter)
        if qualities is not None:
            r = float("inf") if quality_distance is None else quality_distance
            score = icp.evaluate_point_to_line if point_to_line else icp.evaluate
            qualities.append(score(src, transform, r))
        inv = transform.inverse()
        transforms.append(transform)
        inverses.append(inv)
        path.append(inv.t.copy())
    return transforms, inverses, np.array(path).reshape(-1, 2)


class _ArrayPackets:
    """`Scan` (examples/scan3d.rs:17-61) over an in-memory packet array (n_packets, 384, 3)."""

    def __init__(self, packets):
        self.p = np.asarray(packets, dtype=np.float64)

    def size(self):
        return self.p.shape[0]

    def get_range(self, start, end):
        return self.p[start:end].reshape(-1, 3)


def _packet_source(packets):
    return packets if hasattr(packets, "get_range") and hasattr(packets, "size") else _ArrayPackets(packets)


def run_scan3d(packets, step=PACKETS_PER_FRAME, max_iter=20, icp_factory=None, pipeline=True, timings=None):
    """examples/scan3d.rs:104-158 on a packet stream -- an in-memory array (n_packets, 384, 3) or a
    `scans.PacketFile` (the reference's `Scan` over scans.hdf5): the source is packets [0, step) with
    invalid returns removed (:104-107, 63-69); every frame takes dst = packets [index, index+step),
    filtered, THEN advances index (:113-121) -- so the first frame registers the source against itself;
    Icp3d::new(&dst); estimate warm-started (:130-131); path of transform.inverse().t (:133,144).

    `pipeline`: frame k+1's packets are read and filtered, uploaded and its
    search structure built (`Icp3d::new`) by a second host thread on that handle's own stream WHILE frame
    k estimates -- a ring of two handles; the registration itself is untouched, so the trajectory is the
    same bit for bit.  `timings` (optional list) receives the wall time of every frame in seconds.
    Returns (transforms, inverse_transforms, path_xy)."""
    import time
    from concurrent.futures import ThreadPoolExecutor

    icp_factory = icp_factory or Icp3d
    scan = _packet_source(packets)
    src = remove_invalid_values(scan.get_range(0, step))
    transform = Transform.identity()
    transforms, inverses, path = [], [], []

    def make(index):  # what the frame loop does before estimate: Scan::get_range + filter + Icp3d::new
        return icp_factory(remove_invalid_values(scan.get_range(index, index + step)))

    index = 0
    pool = ThreadPoolExecutor(max_workers=1) if pipeline else None
    ahead = pool.submit(make, index) if pool and index + step <= scan.size() else None
    try:
        while index + step <= scan.size():
            t0 = time.perf_counter()
            icp = ahead.result() if ahead is not None else make(index)
            ahead = None
            index += step
            ahead = pool.submit(make, index) if pool and index + step <= scan.size() else None
            transform = icp.estimate(src, transform, max_iter)
            if hasattr(icp, "close"):
                icp.close()  # back to the handle pool: the NEXT make() reuses its buffers and streams
            inv = transform.inverse()
            transforms.append(transform)
            inverses.append(inv)
            path.append(inv.t.copy())
            if timings is not None:
                timings.append(time.perf_counter() - t0)
    finally:
        if pool:
            pool.shutdown(wait=True)
        # (an error above can leave the prefetched handle of the next frame unconsumed)
        if ahead is not None and ahead.done() and ahead.exception() is None and hasattr(ahead.result(), "close"):
            ahead.result().close()
    return transforms, inverses, np.array(path).reshape(-1, 2)


def run_scan_to_map(packets, step=PACKETS_PER_FRAME, max_iter=20, icp_factory=None, max_frames=None,
                    point_to_plane=None, max_correspondence_distance=None, map_radius=None, quality_distance=None,
                    qualities=None, scan_voxel=None, map_voxel=None, scan_outliers=None, scan_voxel_centroids=False):
    """EXTENSION, not in the reference (BASELINE.json configs[4]): the
    scan3d frames registered against a map that grows.  The map starts as frame 0 (filtered as
    examples/scan3d.rs:63-69 does); every later frame is registered against the whole map with
    the reference's own estimator (Icp3d::estimate, warm-started with the previous pose as
    scan3d.rs:131 does) and then appended at its registered pose.  The pose maps the scan into
    the map frame, so the path is its translation directly (no inverse()).
    `icp_factory(dst)` must return an object with .estimate and .append(points, transform).
    `point_to_plane=k` (BASELINE configs[4] names point-to-plane): the frames are registered with the
    point-to-plane residual instead (Icp3d.estimate_point_to_plane, the other labelled extension); every
    map point carries the normal of its k nearest map points AT THE TIME IT WAS INSERTED
    (compute_normals for frame 0, update_normals after every append).
    `max_correspondence_distance=r` (point-to-point only): every frame holds points the map has not seen yet, so
    the frames are registered on the pairs within r of the map (estimate(..., max_correspondence_distance=r),
    include/icp_mi355x.h section 10); None registers as before.
    `map_radius=R` (either residual): a sliding-window map -- after every frame's append (and its update_normals) the
    map is cropped to the xy disc of radius R around the registered position, world.crop(transform.t, R)
    (include/icp_mi355x.h section 11); None calls nothing, so the map grows as before.
    `qualities=[]` (either residual): the quality of every frame's pose against the map it was registered to is
    appended to the list, after the frame's estimate and before its append -- with point_to_plane set,
    world.evaluate_point_to_plane(scan, transform, quality_distance or inf) (a PlaneQuality, include/icp_mi355x.h
    section 13), otherwise world.evaluate(scan, transform, quality_distance or inf) (a Quality, section 9).  None calls
    nothing.
    `scan_voxel=v`: every incoming scan, frame 0 included, is thinned to the first point of every voxel of size v
    (voxel_downsample, include/icp_mi355x.h section 22) before it is registered and appended; None calls nothing.
    `scan_voxel_centroids=True` (needs scan_voxel): every incoming scan, frame 0 included, becomes the means of its
    voxels instead, voxel_centroids(scan, v) (include/icp_mi355x.h section 25): the lower-noise choice for the source
    cloud; False changes nothing and never calls voxel_centroids.
    `map_voxel=v` (either residual): right after every frame's append the map is thinned the same way, world.thin(v):
    the lowest index wins, so every older map point stays and exactly the new points that fall into an occupied voxel
    go -- before update_normals, so that only survivors get a normal, and before the crop; None calls nothing.
    `scan_outliers=(k, std_ratio)`: every incoming scan, frame 0 included, loses its statistical outliers
    (remove_statistical_outliers, include/icp_mi355x.h section 23) after the scan_voxel thinning and before it is
    registered and appended; None calls nothing.
    Returns (transforms, path_xy, map_handle)."""
    if point_to_plane and max_correspondence_distance is not None:
        raise ValueError("max_correspondence_distance applies to the point-to-point registration only")
    if scan_voxel_centroids and scan_voxel is None:
        raise ValueError("scan_voxel_centroids needs scan_voxel, the voxel size")
    icp_factory = icp_factory or Icp3d
    packets = np.asarray(packets, dtype=np.float64)

    def frame(first):
        scan = remove_invalid_values(packets[first:first + step])
        if scan_voxel is not None:
            scan = voxel_centroids(scan, scan_voxel) if scan_voxel_centroids else voxel_downsample(scan, scan_voxel)
        if scan_outliers is not None:
            scan = remove_statistical_outliers(scan, scan_outliers[0], scan_outliers[1])
        return scan

    world = icp_factory(frame(0))
    if point_to_plane:
        world.compute_normals(point_to_plane)
    transform = Transform.identity()
    transforms, path = [], []
    index = step
    while index + step <= packets.shape[0] and (max_frames is None or len(transforms) < max_frames):
        scan = frame(index)
        index += step
        if point_to_plane:
            transform = world.estimate_point_to_plane(scan, transform, max_iter)
        elif max_correspondence_distance is not None:
            transform = world.estimate(scan, transform, max_iter,
                                       max_correspondence_distance=max_correspondence_distance)
        else:
            transform = world.estimate(scan, transform, max_iter)
        if qualities is not None:
            bound = quality_distance or float("inf")
            if point_to_plane:
                qualities.append(world.evaluate_point_to_plane(scan, transform, bound))
            else:
                qualities.append(world.evaluate(scan, transform, bound))
        world.append(scan, transform)
        if map_voxel is not None:
            world.thin(map_voxel)
        if point_to_plane:
            world.update_normals(point_to_plane)
        if map_radius is not None:
            world.crop(transform.t, map_radius)
        transforms.append(transform)
        path.append(transform.t.copy())
    return transforms, np.array(path).reshape(-1, 2), world


def main(argv=None):
    """Headless stand-ins for the reference's two example binaries: the trajectory they draw,
    printed.  `scan2d DIR` reads DIR/001.txt, 002.txt, ... (examples/scan2d.rs); `scan3d` runs the
    synthetic packet stream in the scans.hdf5 layout (the file itself is absent from the reference
    mount); `scan2map` is the growing-map extension on the same stream."""
    import argparse

    from . import synth

    ap = argparse.ArgumentParser(prog="python -m icp_rust_amd.harness", description=main.__doc__)
    ap.add_argument("loop", choices=["scan2d", "scan3d", "scan2map", "write-synth"])
    ap.add_argument("scan_dir", nargs="?", help="scan2d: directory with 001.txt, 002.txt, ...; scan3d / scan2map / "
                                                "write-synth: packet container file")
    ap.add_argument("--frames", type=int, default=8, help="scan3d / scan2map: synthetic frames")
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--point-to-plane", type=int, default=0, metavar="K",
                    help="scan2map: register with point-to-plane residuals, normals from K nearest map points (extension)")
    ap.add_argument("--point-to-line", type=int, default=0, metavar="K",
                    help="scan2d: register with point-to-line residuals, line normals from K nearest targets (extension)")
    ap.add_argument("--map-radius", type=float, default=None, metavar="R",
                    help="scan2map: keep the map within R of the registered position (sliding window, extension)")
    ap.add_argument("--scan-voxel", type=float, default=None, metavar="V",
                    help="scan2map: thin every scan to one point per voxel of size V before it is registered (extension)")
    ap.add_argument("--scan-voxel-centroids", action="store_true",
                    help="scan2map: with --scan-voxel, every scan becomes the means of its voxels instead of their first "
                         "points (extension)")
    ap.add_argument("--map-voxel", type=float, default=None, metavar="V",
                    help="scan2map: thin the map to one point per voxel of size V after every append (extension)")
    ap.add_argument("--scan-outliers", nargs=2, default=None, metavar=("K", "RATIO"),
                    help="scan2map: drop every scan's statistical outliers (mean distance to the K nearest points above "
                         "mean + RATIO deviations) before it is registered (extension)")
    args = ap.parse_args(argv)
    if args.scan_voxel_centroids and args.scan_voxel is None:
        ap.error("--scan-voxel-centroids needs --scan-voxel")
    if args.loop == "scan2d":
        if not args.scan_dir:
            ap.error("scan2d needs the scan directory")
        _, _, path = run_scan2d(args.scan_dir, max_iter=args.max_iter, point_to_line=args.point_to_line or None)
    elif args.loop == "write-synth":
        if not args.scan_dir:
            ap.error("write-synth needs the output file")
        write_packets(args.scan_dir, synth.synthetic_scan3d_packets(PACKETS_PER_FRAME * args.frames))
        print(f"# wrote {PACKETS_PER_FRAME * args.frames} packets to {args.scan_dir}")
        return 0
    elif args.loop == "scan3d":
        stream = PacketFile(args.scan_dir) if args.scan_dir else synth.synthetic_scan3d_packets(PACKETS_PER_FRAME * args.frames)
        _, _, path = run_scan3d(stream, max_iter=args.max_iter)
    else:
        stream = PacketFile(args.scan_dir).as_array() if args.scan_dir else \
            synth.synthetic_scan3d_packets(PACKETS_PER_FRAME * (args.frames + 1))
        _, path, world = run_scan_to_map(stream, max_iter=args.max_iter, point_to_plane=args.point_to_plane or None,
                                         map_radius=args.map_radius, scan_voxel=args.scan_voxel,
                                         map_voxel=args.map_voxel, scan_voxel_centroids=args.scan_voxel_centroids,
                                         scan_outliers=(int(args.scan_outliers[0]), float(args.scan_outliers[1]))
                                         if args.scan_outliers else None)
        print(f"# map: {world.target_count} points")
    for k, (x, y) in enumerate(path):
        print(f"{k:4d} {x:+.9f} {y:+.9f}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
