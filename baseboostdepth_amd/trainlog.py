"""The training log (`--train_log text | panels`): progress lines on stdout, scalar records as JSON lines and panels as
PNG files under the run's log folder.

What the reference prints and sends to wandb every `log_frequency` steps (trainer.py:259-284, :667-772), without wandb:

    <log_path>/<mode>/scalars.jsonl              one JSON object per logged step (mode = "train" | "val")
    <log_path>/<mode>/panels/step_<step:08d>.png  the panel `Trainer.log` rendered on the device (`ops.train_panel`)

Only `to_host` touches the device: what a log step needs on the host (the finished picture, the losses, the arg-min
counts) is copied through pinned buffers behind one synchronisation.
"""
import json
import os
import sys
import time

import torch

ARGMIN_KEYS = ("argmin/true_pose", "argmin/error_induced", "argmin/identity")
RULE = "-" * 81


def sec_to_hm_str(t):
    """Seconds -> '02h50m39s' (utils.sec_to_hm_str)."""
    t = int(t)
    s = t % 60
    t //= 60
    return "{:02d}h{:02d}m{:02d}s".format(t // 60, t % 60, s)


def argmin_fractions(counts, cand_names):
    """Share of a batch's pixels won by a true-pose warp, an error-induced warp and an identity map (the auto-mask):
    `counts` = `ops.argmin_hist` of the arg-min map ([B, MAX_CAND], on the host), `cand_names` = `plan.cand_names`."""
    won = {"T": 0, "E": 0, "I": 0}
    for b, names in enumerate(cand_names):
        for k, (kind, _) in enumerate(names):
            won[kind] += int(counts[b][k])
    total = max(sum(won.values()), 1)
    return dict(zip(ARGMIN_KEYS, (won["T"] / total, won["E"] / total, won["I"] / total)))


class TrainLog:
    def __init__(self, log_path, batch_size, out=None):
        self.log_path = log_path
        self.batch_size = batch_size
        self.out = out                     # None: sys.stdout at the time of the call
        self._pinned = {}

    def _print(self, line):
        print(line, file=self.out or sys.stdout, flush=True)

    # ------------------------------------------------------------------ stdout (trainer.py:667-676, :268-281)
    def log_time(self, epoch, batch_idx, step, num_total_steps, duration, loss, start_time, now=None):
        samples_per_sec = self.batch_size / duration
        time_sofar = (time.time() if now is None else now) - start_time
        training_time_left = (num_total_steps / step - 1.0) * time_sofar if step > 0 else 0
        line = ("epoch {:>3} | batch {:>6} | examples/s: {:5.1f} | loss: {:.5f} | time elapsed: {} | time left: {}"
                .format(epoch, batch_idx, samples_per_sec, loss, sec_to_hm_str(time_sofar), sec_to_hm_str(training_time_left)))
        self._print(line)
        return line

    def context(self, epoch, lr, ordering, scales, valid_frames, cutt, to_use):
        self._print("Starting from epoch {} and current learning rate is {}".format(epoch, lr))
        self._print("Ordering: {}".format(ordering))
        self._print("Scales: {}".format(scales))
        self._print("Valid Frames: {}".format(valid_frames))
        self._print("Current Boosting Weight: {}".format(cutt))
        self._print("Omega: {}".format(to_use))

    def rule(self):
        self._print(RULE)

    # ------------------------------------------------------------------ files
    def scalars(self, mode, record):
        """Appends `record` (a flat dict; tensors and numpy scalars become floats) to <log_path>/<mode>/scalars.jsonl."""
        folder = os.path.join(self.log_path, mode)
        os.makedirs(folder, exist_ok=True)
        row = {k: (v if isinstance(v, (int, str)) and not isinstance(v, bool) else float(v)) for k, v in record.items()}
        with open(os.path.join(folder, "scalars.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")
        return row

    def to_host(self, tensors):
        """Host copies of `tensors`: the device ones go through pinned buffers (kept per position, shape and type), all copies
        are queued first and ONE stream synchronisation follows - the log step's only one."""
        out, device = [], None
        for i, t in enumerate(tensors):
            if not t.is_cuda:
                out.append(t)
                continue
            key = (i, tuple(t.shape), t.dtype)
            buf = self._pinned.get(key)
            if buf is None:
                buf = self._pinned[key] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            buf.copy_(t, non_blocking=True)
            device = t.device
            out.append(buf)
        if device is not None:
            torch.cuda.current_stream(device).synchronize()
        return out

    def panel(self, mode, step, image):
        """Writes the uint8 [h, w, 3] panel to <log_path>/<mode>/panels/step_<step:08d>.png; returns the path.  An image
        on the device is copied once, through a pinned buffer (`to_host`)."""
        from PIL import Image
        assert image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3
        host = self.to_host([image])[0]
        folder = os.path.join(self.log_path, mode, "panels")
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, "step_{:08d}.png".format(step))
        Image.fromarray(host.numpy()).save(path)
        return path
