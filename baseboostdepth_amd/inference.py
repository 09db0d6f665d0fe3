"""Single-image depth prediction (the reference's test_simple.py) on the device.

`DepthPredictor.predict` takes uint8 RGB images of any sizes and returns, per image, the magma-coloured disparity at
the image's own size - what test_simple.py writes as `<name>_Base.jpg`.  A batch costs one upload, the Pillow-exact
LANCZOS resize + ToTensor kernels (`imageops.ImagePipeline`), the networks, one `bbd_disp_viz` call (upsampling,
percentile, normalisation and colour map without leaving the device) and one copy of the colours back; the
reference does all of that per image on the host with Pillow, numpy and matplotlib (test_simple.py:124-148).

`DepthPredictor.predict_cloud` returns the coloured point cloud of every image instead (`ops.point_cloud`,
`pointcloud.py`): what `test_simple.py --point_cloud` writes as `<name>_Base.ply`.

`run_cli` is the command line of the repository's root `test_simple.py`.
"""
import argparse
import glob
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import imageops, ops, pointcloud

HOST_THREADS = 8          # decode / save pool; a fixed small number, never the machine's CPU count


class DepthPrediction:
    """Result of one image: `color` uint8 [H,W,3], `vmin`/`vmax` the normalisation range of the scaled disparity,
    and - when asked for - `scaled_disp` fp32 [H,W] and `depth` = 1 / scaled_disp."""

    __slots__ = ("color", "vmin", "vmax", "scaled_disp", "depth")

    def __init__(self, color, vmin, vmax, scaled_disp=None):
        self.color, self.vmin, self.vmax, self.scaled_disp = color, float(vmin), float(vmax), scaled_disp
        self.depth = None if scaled_disp is None else np.float32(1) / scaled_disp


class DepthPredictor:
    def __init__(self, encoder, decoder, feed_height, feed_width, device="cuda:0", min_depth=0.1, max_depth=80.0,
                 batch_size=16, backend=None):
        self.device = torch.device(device)
        self.encoder = encoder.to(self.device).eval()
        self.decoder = decoder.to(self.device).eval()
        self.feed_height, self.feed_width = int(feed_height), int(feed_width)
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self.batch_size = int(batch_size)
        self.backend = backend or ops.default_backend()
        self.pipe = imageops.ImagePipeline(self.device, self.backend)
        self.last_disp = None

    @classmethod
    def from_weights(cls, folder, vit=False, num_layers=18, device="cuda:0", **kw):
        """Loads `encoder.pth` / `depth.pth` of a weights folder as evaluation.evaluate and the reference do
        (test_simple.py:52-93): the feed size is stored inside encoder.pth, foreign keys are filtered out."""
        from . import networks, tuning
        tuning.use_shipped_db()
        folder = os.path.expanduser(folder)
        assert os.path.isdir(folder), "Cannot find a folder at {}".format(folder)
        enc_dict = torch.load(os.path.join(folder, "encoder.pth"), map_location=device)
        height, width = enc_dict["height"], enc_dict["width"]
        if vit:
            from . import networksvit
            encoder = networksvit.mpvit_small(checkpoint=None)
            encoder.num_ch_enc = [64, 128, 216, 288, 288]
            decoder = networksvit.DepthDecoder()
        else:
            encoder = networks.ResnetEncoder(num_layers, False)
            decoder = networks.DepthDecoder(encoder.num_ch_enc)
        own = encoder.state_dict()
        encoder.load_state_dict({k: v for k, v in enc_dict.items() if k in own})
        decoder.load_state_dict(torch.load(os.path.join(folder, "depth.pth"), map_location=device), strict=False)
        return cls(encoder, decoder, height, width, device, **kw)

    def upload(self, images):
        """uint8 HWC RGB arrays of any sizes -> (device buffer holding them back to back, jobs = [(byte offset, h, w,
        False)] as `ImagePipeline.resize` takes them): the one upload of a batch."""
        arrays = [np.ascontiguousarray(im) for im in images]
        jobs, off = [], 0
        for a in arrays:
            assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3, "images are HWC uint8 RGB"
            jobs.append((off, a.shape[0], a.shape[1], False))
            off += a.size
        host = torch.empty(off, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        flat = host.numpy()
        for a, (o, _, _, _) in zip(arrays, jobs):
            flat[o:o + a.size] = a.reshape(-1)
        return host.to(self.device, non_blocking=True), jobs

    def prepare_uploaded(self, src, jobs):
        """The image kernels on an uploaded batch (`upload`): fp32 [n,3,feed_h,feed_w]."""
        n = len(jobs)
        u8 = self.pipe.resize(src, jobs, self.feed_height, self.feed_width)
        x = torch.empty(n, 3, self.feed_height, self.feed_width, dtype=torch.float32, device=self.device)
        self.pipe.to_float(u8, list(range(n)), x, list(range(n)))
        self.pipe.flush()
        return x

    def prepare(self, images):
        """uint8 HWC RGB arrays of any sizes -> fp32 [n,3,feed_h,feed_w] on the device, bit-equal to
        `ToTensor()(pil.resize((feed_w, feed_h), LANCZOS))` of each: one upload, then the image kernels."""
        return self.prepare_uploaded(*self.upload(images))

    def disparity(self, x):
        """Network output ("disp", 0) for prepared inputs, in batches of at most `batch_size`.  Convolutions are asked
        for deterministic algorithms: without that, MIOpen may pick solvers whose sums land in a different order from
        run to run, the disparity moves by an ulp here and there, and now and then a pixel changes its colour bin - the
        same picture would not always give the same file."""
        cudnn = torch.backends.cudnn
        outs, was = [], cudnn.deterministic
        cudnn.deterministic = True
        try:
            for first in range(0, x.shape[0], self.batch_size):
                outs.append(self.decoder(self.encoder(x[first:first + self.batch_size]))[("disp", 0)])
        finally:
            cudnn.deterministic = was
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def predict(self, images, want_float=False, post_process=False):
        """`post_process`: the prepared batch goes through the networks together with its left-right flipped copy and
        the two raw disparities of every image are blended (`ops.post_process_disp`, Monodepth2's flip
        post-processing) before they are coloured; `last_disp` then holds the blend, [n,h,w]."""
        if not len(images):
            return []
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        with torch.no_grad():
            self.encoder.eval()
            self.decoder.eval()
            x = self.prepare(images)
            if post_process:
                disp = ops.post_process_disp(self.disparity(torch.cat((x, torch.flip(x, [3])), 0)), self.backend)
            else:
                disp = self.disparity(x)
            self.last_disp = disp                                              # kept for inspection (tests)
            return self._pictures(disp, sizes, want_float)

    def _pictures(self, disp, sizes, want_float, raw=False):
        """`ops.disp_viz` of network-size maps at the pictures' own sizes, brought to the host in one go: the results."""
        colour, floats, stats = ops.disp_viz(disp, sizes, self.min_depth, self.max_depth, 95.0, want_float, self.backend,
                                             raw=raw)
        buffers = [ops.viz_buffer(colour), stats] + ([ops.viz_buffer(floats)] if want_float else [])
        host = [_to_host(b) for b in buffers]
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        col_h, stats_h = host[0].numpy(), host[1].numpy()
        flt_h = host[2].numpy() if want_float else None
        results, off = [], 0
        for i, (H0, W0) in enumerate(sizes):
            npx = H0 * W0
            col = col_h[3 * off:3 * (off + npx)].reshape(H0, W0, 3)
            sd = flt_h[off:off + npx].reshape(H0, W0) if want_float else None
            results.append(DepthPrediction(col, stats_h[i, 0], stats_h[i, 1], sd))
            off += ops.viz_granule(npx)
        return results

    def predict_uncertainty(self, images, want_float=False):
        """`predict(images, post_process=True)` and what the flip pass knows about it: the batch goes through the networks
        with its flipped copy, ONE `ops.post_process_uncert` launch gives the blended disparities and their disagreement
        |d - flip(d')|.  Returns (results, uncertainties): the results of `predict`, and per image the
        uncertainty map at the picture's own size - `color` magma between its minimum and maximum, `scaled_disp` (with
        `want_float`) the map itself.  `last_disp` holds the blend, `last_uncert` the map at network size."""
        if not len(images):
            return [], []
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        with torch.no_grad():
            self.encoder.eval()
            self.decoder.eval()
            x = self.prepare(images)
            disp, uncert = ops.post_process_uncert(self.disparity(torch.cat((x, torch.flip(x, [3])), 0)), self.backend)
            self.last_disp, self.last_uncert = disp, uncert
            return self._pictures(disp, sizes, want_float), self._pictures(uncert, sizes, want_float, raw=True)

    def _scaled_disparity(self, images, post_process):
        """(uploaded images, the scaled disparity min_disp + (max_disp - min_disp) * disp at network size [n,.,h,w])."""
        self.encoder.eval()
        self.decoder.eval()
        src, jobs = self.upload(images)
        x = self.prepare_uploaded(src, jobs)
        if post_process:
            disp = ops.post_process_disp(self.disparity(torch.cat((x, torch.flip(x, [3])), 0)), self.backend)
        else:
            disp = self.disparity(x)
        self.last_disp = disp
        min_disp, max_disp = 1.0 / self.max_depth, 1.0 / self.min_depth
        return src, min_disp + (max_disp - min_disp) * disp

    def _ground_rows(self, scaled, sizes, inv_K, camera_height, angle_deg, want_mask):
        """`ops.ground_scale` of scaled disparities at network size, with the intrinsics of every image (`inv_K` [3,3] or
        one per image, for the image's own size) brought to the network's map (`pointcloud.intrinsics_at`)."""
        inv_K = np.asarray(inv_K, np.float32)
        inv_K = inv_K[None].repeat(len(sizes), 0) if inv_K.ndim == 2 else inv_K
        at_map = np.stack([pointcloud.intrinsics_at(k, size, scaled.shape[-2:]) for k, size in zip(inv_K, sizes)])
        return ops.ground_scale(scaled, at_map, camera_height=camera_height, angle_deg=angle_deg, pred_is_disp=True,
                                want_mask=want_mask, backend=self.backend)

    def ground_scale(self, images, inv_K=None, camera_height=1.65, angle_deg=5.0, post_process=False, want_mask=False):
        """The metric scale of every image's prediction from the height of the camera above the road
        (`ops.ground_scale` on the scaled disparity at network size): float32 [n, 12] host rows - [0] the median
        ground height in the prediction's units, [1] ground pixels, [2] candidates, [7] the scale: metres = scale /
        scaled disparity, NaN where no ground was found - and, with `want_mask`, (rows, masks) with masks uint8
        [n, feed_h, feed_w] (1 = ground).  `inv_K` as `predict_cloud` takes it."""
        if not len(images):
            return (np.zeros((0, 12), np.float32), np.zeros((0, self.feed_height, self.feed_width), np.uint8)) \
                if want_mask else np.zeros((0, 12), np.float32)
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        if inv_K is None:
            inv_K = np.stack([pointcloud.intrinsics(H0, W0) for H0, W0 in sizes])
        with torch.no_grad():
            _, scaled = self._scaled_disparity(images, post_process)
            rows, mask = self._ground_rows(scaled, sizes, inv_K, camera_height, angle_deg, want_mask)
            host = [_to_host(rows)] + ([_to_host(mask)] if want_mask else [])
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()
        return (host[0].numpy(), host[1].numpy()) if want_mask else host[0].numpy()

    def predict_cloud(self, images, inv_K=None, scale=1.0, max_depth=None, stride=1, post_process=False, view=None,
                      view_size=3, camera_height=None, angle_deg=5.0, ground_mask=False):
        """The coloured point cloud of every image: one structured array (`pointcloud.VERTEX_DTYPE`: x, y, z, red,
        green, blue, alpha) per image, ready for `pointcloud.write_ply`.  The same network pass as `predict`; the
        scaled disparity min_disp + (max_disp - min_disp) * disp at network size goes through ONE `ops.point_cloud`
        call, which resamples it at every `stride`-th pixel of the image's own size (as the evaluation resamples a
        disparity), takes depth = `scale` / disparity (5.4 for stereo-trained weights), back-projects through `inv_K`
        ([3,3] for all images or one per image; default: the KITTI intrinsics scaled to each image,
        `pointcloud.intrinsics`) and colours every point with its pixel of the uploaded image.  Points beyond
        `max_depth` (default: the predictor's `max_depth * scale`) are dropped, as is anything that is not a depth (a
        negative or non-finite value).  There is no near limit: the sigmoid bounds the disparity.

        `view=(yaw, pitch)` in degrees also draws every cloud as its camera sees it after a turn about the point on
        the optical axis at the cloud's median depth (`cloud_views`), every point a square of `view_size` pixels, and
        returns (clouds, pictures): one uint8 [H,W,3] array per image, at the image's size.

        `camera_height` (metres; `scale` must then be 1) makes the clouds metric without ground truth: the scaled
        disparity goes through `ops.ground_scale` (normals within `angle_deg` of the down axis) and its rows, still on
        the device, are the per-image ratio of the export; the default far limit is then 80.0, and an image without
        ground has a NaN ratio and an empty cloud.  The result then ends in one more element, the ground record: a
        dict of `rows` (float32 [n,12] on the host, as `ground_scale` returns them) and `masks` (uint8 [n, feed_h,
        feed_w] with `ground_mask`, else None)."""
        if camera_height is not None and scale != 1.0:
            raise ValueError("predict_cloud: camera_height recovers the scale, so scale must be 1.0, got %r" % (scale,))
        if not len(images):
            out = ([],) + (([],) if view is not None else ()) + \
                ((dict(rows=np.zeros((0, 12), np.float32), masks=None),) if camera_height is not None else ())
            return out[0] if len(out) == 1 else out
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        if inv_K is None:
            inv_K = np.stack([pointcloud.intrinsics(H0, W0) for H0, W0 in sizes])
        if max_depth is not None:
            far = float(max_depth)
        else:
            far = 80.0 if camera_height is not None else self.max_depth * scale
        with torch.no_grad():
            src, scaled = self._scaled_disparity(images, post_process)
            rows = mask = None
            if camera_height is not None:
                rows, mask = self._ground_rows(scaled, sizes, inv_K, camera_height, angle_deg, ground_mask)
            # `upload` packs the images back to back: image i's bytes start at 3x its pixel offset
            cloud = ops.point_cloud(scaled, ops.cloud_rows(sizes), inv_K, rows=rows, rgb=src, stride=stride,
                                    min_depth=0.0, max_depth=far, pred_is_disp=True,
                                    scale_factor=scale, backend=self.backend)
            ground = None
            if rows is not None:                           # queued before the cloud's read-back synchronises the stream
                ground = [_to_host(rows)] + ([_to_host(mask)] if mask is not None else [])
            clouds = pointcloud.cloud_arrays(*cloud)
            out = (clouds,)
            if view is not None:
                out += (cloud_views(cloud, clouds, sizes, inv_K, view, view_size, self.backend),)
            if ground is not None:
                if self.device.type == "cuda":
                    torch.cuda.current_stream(self.device).synchronize()
                out += (dict(rows=ground[0].numpy(), masks=ground[1].numpy() if len(ground) > 1 else None),)
            return out[0] if len(out) == 1 else out


def cloud_views(cloud, clouds, sizes, inv_K, view, size=3, backend=None):
    """Every cloud of an `ops.point_cloud` batch (`cloud` = its vertices, counts, offsets, still on the device) drawn at
    its image's size from the camera turned by `view` = (yaw, pitch) degrees: uint8 [H,W,3] arrays.  The pivot of the
    turn lies on the optical axis at the median depth of the kept points, taken on the host from `clouds`, the copy
    `pointcloud.cloud_arrays` has already read back (the export keeps no median on the device without a metrics row);
    the points themselves are drawn from the device buffer.  One read-back per picture."""
    vertices, counts, offsets = cloud
    inv_K = np.asarray(inv_K, np.float64)
    inv_K = inv_K[None].repeat(len(sizes), 0) if inv_K.ndim == 2 else inv_K
    pictures = []
    for i, (H, W) in enumerate(sizes):
        canvas = pointcloud.Canvas(W, H, vertices.device, backend)
        if len(clouds[i]):
            pivot = float(np.median(clouds[i]["z"].astype(np.float64)))
            V = pointcloud.orbit_view(np.linalg.inv(inv_K[i][:3, :3]), view[0], view[1], pivot)
            end = vertices.numel() if i + 1 == len(sizes) else int(offsets[i + 1]) * pointcloud.CLOUD_VERTEX
            canvas.points(vertices[int(offsets[i]) * pointcloud.CLOUD_VERTEX:end], count=counts[i:i + 1], view=V, size=size)
        pictures.append(canvas.read()[0])
    return pictures


def _to_host(t):
    if not t.is_cuda:
        return t
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    return host


# ---------------------------------------------------------------------------- command line (test_simple.py)
def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Predict depth for one image or a folder of images and save the "
                                                 "colour-mapped disparity as <name>_Base.jpg.")
    parser.add_argument("--image_path", type=str, required=True, help="path to a test image or folder of images")
    parser.add_argument("--save_path", type=str, required=True,
                        help="output folder for a folder of images (created); a single image is written next to itself")
    parser.add_argument("--ext", type=str, default="jpg", help="image extension to search for in a folder")
    parser.add_argument("--vit", action="store_true", help="the weights are a MonoViT model")
    parser.add_argument("--weights", type=str, required=True, help="folder holding encoder.pth and depth.pth")
    parser.add_argument("--save_npy", action="store_true",
                        help="also write <name>_disp.npy: the scaled disparity, float32, at the original size")
    parser.add_argument("--batch_size", type=int, default=16, help="images per device batch")
    parser.add_argument("--post_process", action="store_true",
                        help="blend the prediction with that of the flipped image (Monodepth2's post-processing)")
    parser.add_argument("--uncertainty", action="store_true",
                        help="also write <name>_Base_uncert.jpg: the disagreement of the prediction and the prediction "
                             "of the mirrored image (implies --post_process); with --save_npy also <name>_uncert.npy")
    parser.add_argument("--point_cloud", action="store_true",
                        help="also write <name>_Base.ply: the coloured point cloud of the prediction (binary PLY)")
    parser.add_argument("--cloud_scale", type=float, default=1.0,
                        help="depth = cloud_scale / scaled disparity (5.4 for stereo-trained weights: metres)")
    parser.add_argument("--cloud_max_depth", type=float, default=None,
                        help="points beyond this depth are dropped (default: the model's max depth times cloud_scale)")
    parser.add_argument("--cloud_stride", type=int, default=1, help="export every N-th pixel in both directions")
    parser.add_argument("--cloud_view", type=float, nargs=2, default=None, metavar=("YAW", "PITCH"),
                        help="with --point_cloud: also write <name>_Base_view.png, the cloud seen by the camera turned "
                             "by these degrees about the point at the median depth on its optical axis")
    parser.add_argument("--cloud_view_size", type=int, default=3, choices=[1, 3, 5, 7],
                        help="side of a point's square in the view, in pixels")
    parser.add_argument("--camera_height", type=float, default=None, metavar="METRES",
                        help="with --point_cloud: the height of the camera above the road; the cloud is brought to "
                             "metres by the median height of the pixels found to be ground (no ground truth needed; "
                             "1.65 for KITTI).  Replaces --cloud_scale")
    parser.add_argument("--ground_angle", type=float, default=5.0, metavar="DEG",
                        help="with --camera_height: a pixel is ground when its surface normal lies within this angle "
                             "of the camera's down axis")
    parser.add_argument("--ground_mask", action="store_true",
                        help="with --camera_height: also write <name>_Base_ground.png, the ground pixels at network "
                             "size (0 and 255)")
    camera = parser.add_mutually_exclusive_group()
    camera.add_argument("--fov", type=float, default=None, metavar="DEG",
                        help="horizontal field of view of the camera in degrees (default: the KITTI intrinsics)")
    camera.add_argument("--intrinsics", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"),
                        help="the camera's intrinsics in pixels of the input image")
    parser.epilog = ("Inputs whose names end in _disp.jpg, _Base.jpg or _Base_uncert.jpg are skipped, so that a second run over a "
                     "folder of jpg files does not colour its own outputs.")
    args = parser.parse_args(argv)
    if args.cloud_stride < 1:
        parser.error("--cloud_stride must be at least 1")
    if args.cloud_scale <= 0:
        parser.error("--cloud_scale must be positive")
    if args.cloud_view is not None and not args.point_cloud:
        parser.error("--cloud_view needs --point_cloud")
    if args.camera_height is not None:
        if not args.point_cloud:
            parser.error("--camera_height needs --point_cloud")
        if not args.camera_height > 0:
            parser.error("--camera_height must be positive")
        if args.cloud_scale != 1.0:
            parser.error("--camera_height recovers the scale from the ground: it excludes a --cloud_scale other than 1.0")
    elif args.ground_mask:
        parser.error("--ground_mask needs --camera_height")
    if not 0.0 <= args.ground_angle < 90.0:
        parser.error("--ground_angle must lie in [0, 90) degrees")
    return args


def find_inputs(image_path, save_path, ext):
    """(paths, output directory) by the reference's rules (test_simple.py:103-122) plus the _Base.jpg skip."""
    if os.path.isfile(image_path):
        paths, out_dir = [image_path], os.path.dirname(image_path)
    elif os.path.isdir(image_path):
        paths, out_dir = sorted(glob.glob(os.path.join(image_path, "*.{}".format(ext)))), save_path
    else:
        raise Exception("Can not find args.image_path: {}".format(image_path))
    paths = [p for p in paths if not p.endswith(("_disp.jpg", "_Base.jpg", "_Base_uncert.jpg"))]
    return paths, out_dir


def _load(path):
    import PIL.Image as pil
    with pil.open(path) as im:
        return np.asarray(im.convert("RGB"))


def _save(out_dir, path, result, save_npy):
    import PIL.Image as pil
    stem = os.path.splitext(os.path.basename(path))[0]
    dest = os.path.join(out_dir, "{}_Base.jpg".format(stem))
    pil.fromarray(result.color).save(dest)
    if save_npy:
        np.save(os.path.join(out_dir, "{}_disp.npy".format(stem)), result.scaled_disp)
    return dest


def _save_uncert(out_dir, path, result, save_npy):
    import PIL.Image as pil
    stem = os.path.splitext(os.path.basename(path))[0]
    dest = os.path.join(out_dir, "{}_Base_uncert.jpg".format(stem))
    pil.fromarray(result.color).save(dest)
    if save_npy:
        np.save(os.path.join(out_dir, "{}_uncert.npy".format(stem)), result.scaled_disp)
    return dest


def _save_cloud(out_dir, path, cloud):
    stem = os.path.splitext(os.path.basename(path))[0]
    return pointcloud.write_ply(os.path.join(out_dir, "{}_Base.ply".format(stem)), cloud)


def _save_view(out_dir, path, picture):
    import PIL.Image as pil
    stem = os.path.splitext(os.path.basename(path))[0]
    dest = os.path.join(out_dir, "{}_Base_view.png".format(stem))
    pil.fromarray(picture).save(dest)
    return dest


def _save_ground(out_dir, path, mask):
    import PIL.Image as pil
    stem = os.path.splitext(os.path.basename(path))[0]
    dest = os.path.join(out_dir, "{}_Base_ground.png".format(stem))
    pil.fromarray(np.asarray(mask, np.uint8) * np.uint8(255)).save(dest)
    return dest


def _report_ground(pool, out_dir, paths, ground):
    """One line per image from the ground record of `predict_cloud`, a warning where no ground was found; returns the
    futures of the mask files, where the record holds masks."""
    saves = []
    for i, path in enumerate(paths):
        median, count, candidates, scale = (float(ground["rows"][i][c]) for c in (0, 1, 2, 7))
        name = os.path.basename(path)
        if np.isnan(scale):
            print("   WARNING: {}: no ground found ({:d} ground pixels of {:d} candidates); the cloud is left empty"
                  .format(name, int(count), int(candidates)))
        else:
            print("   {}: scale {:.4f} | median ground height {:.4f} | ground {:.1f}% of {:d} candidates"
                  .format(name, scale, median, 100.0 * count / max(candidates, 1.0), int(candidates)))
        if ground.get("masks") is not None:
            saves.append(pool.submit(_save_ground, out_dir, path, ground["masks"][i]))
    return saves


def _cloud_inv_K(args, images):
    return np.stack([pointcloud.intrinsics(im.shape[0], im.shape[1], fov=getattr(args, "fov", None),
                                           fxfycxcy=getattr(args, "intrinsics", None)) for im in images])


def run_cli(args, predictor=None):
    """Body of test_simple.py.  `predictor` may be injected (tests); by default it is loaded from `args.weights`.
    With `--point_cloud` every batch also goes through `predict_cloud` (a second network pass: `predict` is left as it
    is) and `<name>_Base.ply` is written next to the JPEG; `--cloud_view YAW PITCH` adds `<name>_Base_view.png`.
    `--camera_height METRES` scales every cloud by the camera's height above its ground pixels (`ops.ground_scale`),
    prints the scale, the median ground height and the ground share of every image - a warning where no ground was
    found - and, with `--ground_mask`, writes `<name>_Base_ground.png`.
    Returns the list of written JPEG paths."""
    paths, out_dir = find_inputs(args.image_path, args.save_path, args.ext)
    if predictor is None:
        print("-> Loading model from ", args.weights)
        predictor = DepthPredictor.from_weights(args.weights, vit=args.vit, batch_size=args.batch_size)
    print("-> Predicting on {:d} test images".format(len(paths)))
    if out_dir and not os.path.exists(out_dir):
        os.makedirs(out_dir)
    out_dir = out_dir or "."
    batch = max(1, int(getattr(args, "batch_size", 16)))
    written, pending, cloud_saves = [], [], []
    with ThreadPoolExecutor(max_workers=HOST_THREADS) as pool:
        chunks = [paths[i:i + batch] for i in range(0, len(paths), batch)]
        loads = [pool.map(_load, c) for c in chunks[:1]]                 # decode runs one batch ahead
        for k, chunk in enumerate(chunks):
            images = list(loads[k])
            if k + 1 < len(chunks):
                loads.append(pool.map(_load, chunks[k + 1]))
            if getattr(args, "uncertainty", False):         # an injected predictor meets the method only when it is set
                results, uncerts = predictor.predict_uncertainty(images, want_float=args.save_npy)
                cloud_saves += [pool.submit(_save_uncert, out_dir, p, u, args.save_npy) for p, u in zip(chunk, uncerts)]
            elif getattr(args, "post_process", False):      # an injected predictor meets the keyword only when it is set
                results = predictor.predict(images, want_float=args.save_npy, post_process=True)
            else:
                results = predictor.predict(images, want_float=args.save_npy)
            pending += [pool.submit(_save, out_dir, p, r, args.save_npy) for p, r in zip(chunk, results)]
            if getattr(args, "point_cloud", False):
                kw = dict(inv_K=_cloud_inv_K(args, images), scale=args.cloud_scale, max_depth=args.cloud_max_depth,
                          stride=args.cloud_stride,
                          post_process=bool(getattr(args, "post_process", False) or getattr(args, "uncertainty", False)))
                if getattr(args, "cloud_view", None) is not None:        # as above: the keywords only when they are set
                    kw.update(view=tuple(args.cloud_view), view_size=getattr(args, "cloud_view_size", 3))
                camera_height = getattr(args, "camera_height", None)
                if camera_height is not None:
                    kw.update(camera_height=camera_height, angle_deg=getattr(args, "ground_angle", 5.0),
                              ground_mask=bool(getattr(args, "ground_mask", False)))
                result = predictor.predict_cloud(images, **kw)
                result = result if isinstance(result, tuple) else (result,)
                clouds = result[0]
                if "view" in kw:
                    cloud_saves += [pool.submit(_save_view, out_dir, p, v) for p, v in zip(chunk, result[1])]
                if camera_height is not None:
                    cloud_saves += _report_ground(pool, out_dir, chunk, result[-1])
                cloud_saves += [pool.submit(_save_cloud, out_dir, p, c) for p, c in zip(chunk, clouds)]
        written = [f.result() for f in pending]
        for f in cloud_saves:
            f.result()
    print("-> Done!")
    return written


def main(argv=None):
    return run_cli(parse_args(argv))
