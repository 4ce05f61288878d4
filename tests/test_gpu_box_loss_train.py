"""training.train_step with validation.YOLOLossV3(box_loss="ciou") on the real network: a seeded YoloFastest at a 64x96 input, one fixed
batch of 4 frames with 3 boxes each, 60 iterations of training.Adam(lr=1e-3) -- alone, and with branch_weight and ModelEMA (train_step
itself is unchanged; this shows the three compose).  Every loss of every step is finite, positions 2..4 of the tuple stay zero, and the
box term after the last step is below the one after the first."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 60


def _setup(dev):
    import yolo_fastest_amd as yf
    io = copy.deepcopy(yf.io_params_for(256))
    io.update(input_shape=[64, 96, 1], origin_img_shape=[64, 96, 1])
    torch.manual_seed(5)
    m = yf.YoloFastest(io)
    m.initialize_weights()
    m = m.to(dev).train()
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(4, 1, 64, 96, generator=g) - 0.5).to(dev)
    rng = np.random.default_rng(9)
    t = np.zeros((4, 8, 6), np.float32)
    t[:, :3, 0:2] = rng.uniform(0.1, 0.9, (4, 3, 2))
    t[:, :3, 2:4] = rng.uniform(0.08, 0.5, (4, 3, 2))
    t[:, :3, 4] = rng.integers(0, io["num_cls"], (4, 3))
    t[:, :3, 5] = 255.0
    return io, m, x, torch.from_numpy(t).to(dev)


@pytest.mark.parametrize("composed", [False, True], ids=["alone", "branch_weight+ema"])
def test_sixty_steps_with_ciou(composed):
    from yolo_fastest_amd import training, validation as val
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    io, m, x, targets = _setup(dev)
    crit = [val.YOLOLossV3(io["anchors"][i], io["num_cls"], io["input_shape"], dev, model=m, box_loss="ciou") for i in range(2)]
    opt = training.Adam(m.parameters(), lr=1e-3)
    ema = training.ModelEMA(m) if composed else None
    weights = [0.5, 1.5] if composed else None
    box = []
    for _ in range(STEPS):
        losses = training.train_step(m, crit, opt, x, targets, weights, ema=ema)
        vals = [float(losses[0].detach())] + [float(v) for v in losses[1:]]
        assert len(vals) == 7 and all(math.isfinite(v) for v in vals), vals
        assert vals[2:5] == [0.0, 0.0, 0.0]
        box.append(vals[1])
    assert 0 < box[-1] < box[0], (box[0], box[-1])
    if composed:
        assert ema.updates == STEPS
