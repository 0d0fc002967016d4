"""The synthetic clip and model of the fine-tuning tests (host and GPU files share them)."""
import io

import numpy as np

from rrin_amd import Net, y4m
from rrin_amd.synthetic import keyed_state_dict

# the fixed-batch descent test, on the CPU and on the GPU with the same parameters: a 3-frame clip
# has one triplet (0, 1, 2); 8 steps of AdamW at the reference's 1e-4 descend on the CPU with the
# keyed synthetic weights (the losses are in DESIGN.md), so no other rate was needed
DESCENT = {"steps": 8, "lr": 1e-4, "batch": 1, "crop": 32, "augment": False, "val_fraction": 0.0}


def clip_bytes(w, h, n):
    """An n-frame w x h 8-bit 4:2:0 Y4M stream: a smooth pattern that moves two pixels a frame."""
    buf = io.BytesIO()
    wr = y4m.Writer(buf, w, h, 24, 1)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    for k in range(n):
        y = np.clip((0.5 + 0.25 * np.sin((xx - 2 * k) / 5.0) + 0.2 * np.cos((yy + 2 * k) / 7.0)) * 255, 0, 255)
        u = np.clip(128 + 40 * np.sin((cx - k) / 4.0), 0, 255)
        v = np.clip(128 + 40 * np.cos((cy + k) / 6.0), 0, 255)
        wr.write(np.concatenate([p.astype(np.uint8).ravel() for p in (y, u, v)]))
    return buf.getvalue()


def keyed_net(device="cpu"):
    net = Net()
    net.load_state_dict(keyed_state_dict(net.state_dict(), stress=False))
    return net.to(device)
