"""Checkpoint comparison sheets (the reference's validation.py) on the device.

For every frame of a split the reference's authors looked at the input picture, the LiDAR ground truth and every
ablation checkpoint's disparity side by side, with a per-frame abs_rel per checkpoint.  `compare_batch` does that for a
batch of frames without leaving the device: one upload of the decoded pictures, the Pillow-exact LANCZOS resize +
ToTensor kernels once per distinct feed size, per model the networks, one `bbd_disp_viz` (raw disparity, min-max
normalised: validation.py:205-212), one `bbd_depth_metrics` (validation.py:232-269) and optionally one `bbd_error_map`,
one `bbd_gt_viz` (validation.py:250-254), the resize launches that bring every picture to the cell size, tensor slicing
into the sheets, and one synchronisation with the host (`CompareBatch.host`).

`run_cli` is the command line of the repository's root `validation.py`.
"""
import argparse
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import inference, ops
from .evaluation import GroundTruthSet, depth_metrics
from .layers import disp_to_depth

MIN_DEPTH, MAX_DEPTH = 0.1, 80.0            # validation.py:175-176 (evaluate_depth.py scores from 1e-3)
CELL = (188, 621)                           # rows, columns: the reference's scale=w=621 at KITTI's aspect ratio


# ---------------------------------------------------------------------------- sheet layout
def sheet_rows(n_models, error_maps=False):
    """Rows of cells: [input | ground truth], then the models two per row, or one per row with its error map."""
    return 1 + (n_models if error_maps else (n_models + 1) // 2)


def sheet_cells(n_models, error_maps=False):
    """{(row, column): (kind, model)} with kind "image" | "gt" | "disp" | "error"; cells not named are black."""
    cells = {(0, 0): ("image", None), (0, 1): ("gt", None)}
    for m in range(n_models):
        if error_maps:
            cells[(1 + m, 0)] = ("disp", m)
            cells[(1 + m, 1)] = ("error", m)
        else:
            cells[(1 + m // 2, m % 2)] = ("disp", m)
    return cells


def cell_rect(row, col, cell=CELL):
    """(y0, y1, x0, x1) of a cell in the sheet."""
    ch, cw = cell
    return row * ch, (row + 1) * ch, col * cw, (col + 1) * cw


def sheet_labels(names, abs_rel, error_maps=False):
    """{(row, column): text} for one frame: `Images`, `Depth`, `<MODEL upper-case> <abs_rel %.3f>` on the disparities."""
    labels = {(0, 0): "Images", (0, 1): "Depth"}
    for (row, col), (kind, m) in sheet_cells(len(names), error_maps).items():
        if kind == "disp":
            labels[(row, col)] = "%s %.3f" % (str(names[m]).upper(), float(abs_rel[m]))
    return labels


def _bitmap_font():
    """Pillow's built-in bitmap font (newer Pillow versions answer `load_default()` with a scalable one)."""
    from PIL import ImageFont
    return getattr(ImageFont, "load_default_imagefont", ImageFont.load_default)()


def label_boxes(labels, cell=CELL):
    """{(row, column): (y0, y1, x0, x1)}: the pixels `label_sheet` may touch - the text's box at (10, 10) of its cell,
    clipped to the cell."""
    font = _bitmap_font()
    boxes = {}
    for (row, col), text in labels.items():
        y0, y1, x0, x1 = cell_rect(row, col, cell)
        l, t, r, b = font.getbbox(text)
        boxes[(row, col)] = (min(y0 + 10 + t, y1), min(y0 + 10 + b, y1), min(x0 + 10 + l, x1), min(x0 + 10 + r, x1))
    return boxes


def label_sheet(sheet, labels, cell=CELL):
    """White text at (10, 10) of each labelled cell in Pillow's built-in bitmap font, drawn on the host into a copy of
    `sheet` (uint8 [H,W,3]); nothing outside `label_boxes` changes."""
    from PIL import Image, ImageDraw
    font = _bitmap_font()
    out = np.array(sheet, copy=True)
    for (row, col), text in labels.items():
        y0, y1, x0, x1 = cell_rect(row, col, cell)
        tile = Image.fromarray(out[y0:y1, x0:x1])               # drawn per cell: text never runs into a neighbour
        ImageDraw.Draw(tile).text((10, 10), text, fill=(255, 255, 255), font=font)
        out[y0:y1, x0:x1] = np.asarray(tile)
    return out


# ---------------------------------------------------------------------------- one batch on the device
class CompareBatch:
    """What `compare_batch` returns, on the device: `sheets` uint8 [n, rows*ch, 2*cw, 3] (unlabelled), `disps[m][i]`
    uint8 [H0,W0,3], `gt[i]` uint8 [GH,GW,3], `errors[m][i]` uint8 [GH,GW,3] (None without error maps) and `rows` fp32
    [M, n, 12], the `depth_metrics` rows of every model.  `host()` brings all of it over with one synchronisation."""

    def __init__(self, sheets, disps, gt, errors, rows):
        self.sheets, self.disps, self.gt, self.errors, self.rows = sheets, disps, gt, errors, rows

    def host(self):
        groups = [[self.sheets[i] for i in range(self.sheets.shape[0])], self.gt] + list(self.disps) + \
                 (list(self.errors) if self.errors is not None else [])
        flat = torch.cat([t.reshape(-1) for g in groups for t in g])
        staged = [inference._to_host(flat), inference._to_host(self.rows)]
        if flat.is_cuda:
            torch.cuda.current_stream(flat.device).synchronize()
        bytes_h, off, out = staged[0].numpy(), 0, []
        for g in groups:
            views = []
            for t in g:
                views.append(bytes_h[off:off + t.numel()].reshape(tuple(t.shape)))
                off += t.numel()
            out.append(views)
        M = len(self.disps)
        errors = out[2 + M:] if self.errors is not None else None
        return CompareBatch(np.stack(out[0]), out[2:2 + M], out[1], errors, staged[1].numpy())


def _background(src, jobs, batch, pipe):
    """The input pictures where `bbd_error_map` reads them: at the ground-truth sizes, packed like the maps.  A batch of
    consecutive frames whose pictures have their maps' sizes - KITTI - is the uploaded buffer itself."""
    if all((h, w) == s and off == 3 * r for (off, h, w, _), s, r in zip(jobs, batch.shapes, batch.rel)):
        return src
    pictures = []
    for job, (gh, gw) in zip(jobs, batch.shapes):
        pictures.append(pipe.resize(src, [job], gh, gw)[0])
    pipe.flush()
    return pictures


def compare_batch(images, gts, indices, predictors, cell=CELL, error_maps=False, err_max=0.5, radius=2, backend=None):
    """One batch of frames against `predictors` (a list of `inference.DepthPredictor` on one device): `images` are
    uint8 HWC RGB arrays of any sizes, frame i is scored against `gts[indices[i]]`.  Returns a `CompareBatch` of device
    tensors; nothing synchronises with the host."""
    assert len(predictors) > 0 and len(images) == len(indices) and len(images) > 0
    first = predictors[0]
    backend = backend or first.backend
    n, M = len(images), len(predictors)
    ch, cw = int(cell[0]), int(cell[1])
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    batch = ops._GtBatch(gts, indices)
    with torch.no_grad():
        src, jobs = first.upload(images)
        prepared, disps, errors, rows, cells = {}, [], [], [], {}
        pipe = first.pipe
        for p in predictors:
            key = (p.feed_height, p.feed_width)
            if key not in prepared:
                prepared[key] = p.prepare_uploaded(src, jobs)
        background = _background(src, jobs, batch, pipe) if error_maps else None
        for m, p in enumerate(predictors):
            p.encoder.eval()
            p.decoder.eval()
            disp = p.disparity(prepared[(p.feed_height, p.feed_width)])
            colour, _, _ = ops.disp_viz(disp, sizes, raw=True, backend=backend)
            pred_disp, _ = disp_to_depth(disp, MIN_DEPTH, MAX_DEPTH)
            r = depth_metrics(pred_disp, gts, batch.idx, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, pred_is_disp=True,
                              median="numpy", backend=backend)
            disps.append(colour)
            rows.append(r)
            buf, off = ops.viz_buffer(colour), 0
            picks = []
            for H0, W0 in sizes:
                picks.append((3 * off, H0, W0, False))
                off += ops.viz_granule(H0 * W0)
            cells[("disp", m)] = pipe.resize(buf, picks, ch, cw)
            if error_maps:
                err, _ = ops.error_map(pred_disp, gts, batch.idx, r, images=background, min_depth=MIN_DEPTH,
                                       max_depth=MAX_DEPTH, err_max=err_max, radius=radius, backend=backend)
                errors.append(err)
                cells[("error", m)] = pipe.resize(ops.viz_buffer(err), _gt_jobs(batch), ch, cw)
        gt_pictures, _ = ops.gt_viz(gts, batch.idx, max_inv=MAX_DEPTH, backend=backend)
        cells[("gt", None)] = pipe.resize(ops.viz_buffer(gt_pictures), _gt_jobs(batch), ch, cw)
        cells[("image", None)] = pipe.resize(src, jobs, ch, cw)
        pipe.flush()
        R = sheet_rows(M, error_maps)
        sheets = torch.zeros(n, R * ch, 2 * cw, 3, dtype=torch.uint8, device=src.device)
        for (row, col), key in sheet_cells(M, error_maps).items():
            y0, y1, x0, x1 = cell_rect(row, col, (ch, cw))
            sheets[:, y0:y1, x0:x1] = cells[key]
    return CompareBatch(sheets, disps, gt_pictures, errors if error_maps else None, torch.stack(rows))


def _gt_jobs(batch):
    return [(3 * r, gh, gw, False) for r, (gh, gw) in zip(batch.rel, batch.shapes)]


# ---------------------------------------------------------------------------- command line (validation.py)
def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Compare checkpoints frame by frame: input, ground truth and every "
                                                 "model's disparity side by side, with a per-frame abs_rel.")
    parser.add_argument("--model_name", nargs="+", default=[], help="checkpoint folders under --models_dir (or paths)")
    parser.add_argument("--models_dir", type=str, default=".", help="folder holding one folder per model")
    parser.add_argument("--kt_path", type=str, required=True, help="KITTI raw root")
    parser.add_argument("--split_dir", type=str, default=os.path.join("splits", "eigen_zhou"))
    parser.add_argument("--files", type=str, default="val_files.txt", help="frame list inside --split_dir")
    parser.add_argument("--output", type=str, default="validation_vis")
    parser.add_argument("--ViT", action="store_true", help="the weights are MonoViT models (all of them)")
    parser.add_argument("--num_layers", type=int, default=18)
    parser.add_argument("--ext", type=str, default="jpg", help="image extension of the frames")
    parser.add_argument("--format", type=str, default="jpg", choices=["jpg", "png"], help="format of the written pictures")
    parser.add_argument("--cell_size", type=int, nargs=2, default=[CELL[1], CELL[0]], metavar=("WIDTH", "HEIGHT"))
    parser.add_argument("--error_maps", action="store_true", help="one row per model: disparity | error map")
    parser.add_argument("--err_max", type=float, default=0.5, help="abs_rel at which the error map saturates")
    parser.add_argument("--dot_radius", type=int, default=2, help="radius of an error map's dots (0-4)")
    parser.add_argument("--no_labels", action="store_true", help="leave the sheets as the device wrote them")
    parser.add_argument("--batch_size", type=int, default=16, help="frames per device batch")
    parser.add_argument("--limit", type=int, default=None, help="only the first N frames")
    for flag in ("--SQL", "--pred_metric_depth"):
        parser.add_argument(flag, action="store_true", help="not part of this build")
    args = parser.parse_args(argv)
    bad = [f for f in ("--SQL", "--pred_metric_depth") if getattr(args, f[2:])]
    if bad:
        parser.error("%s select parts of the reference that are outside this build's scope" % ", ".join(bad))
    if not args.model_name:
        parser.error("--model_name needs at least one model")
    if not 0 <= args.dot_radius <= 4:
        parser.error("--dot_radius must be 0 ... 4")
    if min(args.cell_size) < 1 or args.batch_size < 1:
        parser.error("--cell_size and --batch_size must be positive")
    return args


def frame_token(token):
    """An all-digit frame token shorter than 10 characters is zero-padded to 10 (KITTI's file names)."""
    return token.zfill(10) if token.isdigit() and len(token) < 10 else token


def read_frames(split_dir, files, kt_path, ext="jpg", limit=None):
    """[(folder, frame, picture path)] of the split's lines: first token the folder, second the frame; the picture is
    always image_02 (validation.py:293-296)."""
    with open(os.path.join(split_dir, files)) as f:
        lines = [line.split() for line in f.read().splitlines() if line.strip()]
    frames = []
    for t in lines[:limit]:
        if len(t) < 2:
            raise ValueError("%s: a line needs a folder and a frame, got %r" % (files, " ".join(t)))
        frame = frame_token(t[1])
        frames.append((t[0], frame, os.path.join(kt_path, t[0], "image_02", "data", "%s.%s" % (frame, ext))))
    return frames


def model_folder(models_dir, name):
    return name if os.path.isdir(name) else os.path.join(models_dir, name)


def load_ground_truth(split_dir, frames, kt_path, device):
    """`gt_depths.npz` of the split; where it is missing and every frame token is a number, the maps are projected from
    the Velodyne scans on the device, as `evaluation._evaluate_kitti` does."""
    gt_path = os.path.join(split_dir, "gt_depths.npz")
    if os.path.isfile(gt_path):
        data = np.load(gt_path, fix_imports=True, encoding="latin1", allow_pickle=True)["data"]
        return GroundTruthSet(data, device)
    if not all(frame.isdigit() for _, frame, _ in frames):
        raise FileNotFoundError("%s not found, and the frame list does not name Velodyne scans" % gt_path)
    from . import kitti_utils
    print("-> %s not found: ground truth of %d frames projected from the Velodyne scans under %s on the device"
          % (gt_path, len(frames), kt_path))
    triples = [(os.path.join(kt_path, folder.split("/")[0]),
                os.path.join(kt_path, folder, "velodyne_points/data", "{:010d}.bin".format(int(frame))), 2)
               for folder, frame, _ in frames]
    return kitti_utils.generate_depth_maps(triples, device, vel_depth=True)


def write_csv(path, names, frames, abs_rel):
    """`index,frame,<model>...`, one row per frame with %.6f values, a last row `mean` (abs_rel is [frames, models])."""
    abs_rel = np.asarray(abs_rel, dtype=np.float64).reshape(len(frames), len(names))
    with open(path, "w") as f:
        f.write(",".join(["index", "frame"] + [str(n) for n in names]) + "\n")
        for i, (folder, frame, _) in enumerate(frames):
            f.write(",".join(["%010d" % i, "%s/%s" % (folder, frame)] + ["%.6f" % v for v in abs_rel[i]]) + "\n")
        f.write(",".join(["mean", ""] + ["%.6f" % v for v in abs_rel.mean(0)]) + "\n")


def _save(path, array):
    import PIL.Image as pil
    pil.fromarray(array).save(path)
    return path


def run_cli(args, predictors=None, gts=None):
    """Body of validation.py.  `predictors` (one `DepthPredictor` per --model_name) and `gts` (a `GroundTruthSet`) may
    be injected (tests).  Returns (abs_rel [frames, models], ratios [frames, models])."""
    names = list(args.model_name)
    cell = (int(args.cell_size[1]), int(args.cell_size[0]))
    frames = read_frames(args.split_dir, args.files, args.kt_path, args.ext, args.limit)
    if predictors is None:
        predictors = []
        for name in names:
            folder = model_folder(args.models_dir, name)
            print("-> Loading model from ", folder)
            predictors.append(inference.DepthPredictor.from_weights(folder, vit=args.ViT, num_layers=args.num_layers,
                                                                    batch_size=args.batch_size))
    assert len(predictors) == len(names)
    if gts is None:
        gts = load_ground_truth(args.split_dir, frames, args.kt_path, predictors[0].device)
    if len(gts) < len(frames) or (args.limit is None and len(gts) != len(frames)):
        raise ValueError("%s lists %d frames, the ground truth holds %d maps" % (args.files, len(frames), len(gts)))
    folders = ["depth", "sheets"] + [os.path.basename(os.path.normpath(n)) for n in names]
    stems = folders[2:]
    if args.error_maps:
        folders += [os.path.join("errors", s) for s in stems]
    for d in folders:
        os.makedirs(os.path.join(args.output, d), exist_ok=True)
    print("-> Comparing {:d} models on {:d} frames".format(len(names), len(frames)))
    batch = max(1, int(args.batch_size))
    abs_rel, ratios, pending = [], [], []
    with ThreadPoolExecutor(max_workers=inference.HOST_THREADS) as pool:
        chunks = [list(range(i, min(i + batch, len(frames)))) for i in range(0, len(frames), batch)]
        loads = [pool.map(inference._load, [frames[i][2] for i in c]) for c in chunks[:1]]    # decode runs one batch ahead
        for k, chunk in enumerate(chunks):
            images = list(loads[k])
            if k + 1 < len(chunks):
                loads.append(pool.map(inference._load, [frames[i][2] for i in chunks[k + 1]]))
            res = compare_batch(images, gts, chunk, predictors, cell=cell, error_maps=args.error_maps,
                                err_max=args.err_max, radius=args.dot_radius).host()
            abs_rel.append(res.rows[:, :, 0].T)
            ratios.append(res.rows[:, :, 7].T)
            for j, i in enumerate(chunk):
                name = "%010d.%s" % (i, args.format)
                sheet = res.sheets[j]
                if not args.no_labels:
                    sheet = label_sheet(sheet, sheet_labels(stems, res.rows[:, j, 0], args.error_maps), cell)
                pending.append(pool.submit(_save, os.path.join(args.output, "sheets", name), sheet))
                pending.append(pool.submit(_save, os.path.join(args.output, "depth", name), res.gt[j]))
                for m, stem in enumerate(stems):
                    pending.append(pool.submit(_save, os.path.join(args.output, stem, name), res.disps[m][j]))
                    if args.error_maps:
                        pending.append(pool.submit(_save, os.path.join(args.output, "errors", stem, name), res.errors[m][j]))
        for f in pending:
            f.result()
    abs_rel = np.concatenate(abs_rel).astype(np.float64) if abs_rel else np.zeros((0, len(names)))
    ratios = np.concatenate(ratios).astype(np.float64) if ratios else np.zeros((0, len(names)))
    write_csv(os.path.join(args.output, "abs_rel.csv"), stems, frames, abs_rel)
    for m, stem in enumerate(stems):
        print("   {:<24} abs_rel {:0.4f} | scaling ratio {:0.4f}".format(stem, abs_rel[:, m].mean(), ratios[:, m].mean()))
    print("-> Done!")
    return abs_rel, ratios


def main(argv=None):
    return run_cli(parse_args(argv))
