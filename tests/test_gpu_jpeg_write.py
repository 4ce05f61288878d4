"""plot.draw_boxes_device against plot.plot_one_box applied in order, and Detect_YOLO(..., write="device") against write="host": the
same files byte for byte, the same labels and log lines.  The yardsticks are plot_one_box and `_save` as the host path runs them."""
import logging
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import test_cpu_draw as dc  # noqa: E402

WDIR = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights")
DATA = os.path.join(HERE, "golden", "test_data")
WEIGHTS = {256: "yolo_fastest_256x320_epoch28.pth", 512: "yolo_fastest_512x640_epoch27.pth"}


@pytest.fixture(scope="module")
def yf():
    import yolo_fastest_amd
    return yolo_fastest_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("tl", dc.THICKNESS)
def test_draw_boxes_device_equals_plot_one_box_on_every_case(dev, tl, order):
    """All cases of tests/test_cpu_draw.py as the frames of one batch, plus a frame without boxes."""
    from yolo_fastest_amd import plot
    want = [dc.background(k) for k in range(len(dc.CASES))] + [dc.background(99)]
    frames = np.stack(want).copy()
    for k, (_, boxes) in enumerate(dc.CASES):
        for xyxy, label, ci in boxes:
            plot.plot_one_box(xyxy, want[k], color=dc.COLORS[ci], label=label, line_thickness=tl)
    boxes = [[b[0] for b in c[1]] for c in dc.CASES] + [[]]
    labels = [[b[1] for b in c[1]] for c in dc.CASES] + [[]]
    colors = [[dc.COLORS[b[2]] for b in c[1]] for c in dc.CASES] + [[]]
    d = torch.from_numpy(frames if order == "rgb" else np.ascontiguousarray(frames[..., ::-1])).to(dev)
    got = plot.draw_boxes_device(d, boxes, labels, colors, line_thickness=tl, order=order).cpu().numpy()
    got = got if order == "rgb" else got[..., ::-1]
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), (k, tl, order, int((got[k] != want[k]).any(axis=2).sum()))


@pytest.mark.parametrize("net", [256, 512])
def test_draw_boxes_device_on_the_real_detections_of_the_bundled_frames(yf, dev, net):
    from yolo_fastest_amd import plot
    io = yf.io_params_for(net)
    det = yf.Detect_YOLO(dev, os.path.join(WDIR, WEIGHTS[net]), {"io_params": io}, logging.getLogger("draw-real"))
    names = sorted(os.listdir(DATA))
    rgb = [np.asarray(Image.open(os.path.join(DATA, n)).convert("RGB")) for n in names]
    bgr = torch.from_numpy(np.stack(rgb)[..., ::-1].copy()).to(dev)
    results = det.detect_bgr_u8(bgr)
    assert sum(len(r) for r in results) >= 10
    want = [a.copy() for a in rgb]
    labels = [det._labels(r) for r in results]
    for f, r in enumerate(results):
        assert det._save(None, want[f], r) == labels[f]
        for (*xyxy, conf, cls_score, cls_pred), lab in zip(r, labels[f]):
            plot.plot_one_box(xyxy, want[f], label=lab, color=det.colors[int(cls_pred) % 3], line_thickness=3)
    frames = bgr.clone()
    plot.draw_boxes_device(frames, [[b[:4] for b in r] for r in results], labels, [[det.colors[int(b[6]) % 3] for b in r] for r in results],
                           line_thickness=3, order="bgr")
    got = frames.cpu().numpy()[..., ::-1]
    for f in range(len(names)):
        assert np.array_equal(got[f], want[f]), names[f]


def test_draw_boxes_device_checks_its_arguments(dev):
    from yolo_fastest_amd import plot
    f = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=dev)
    for frames, boxes in ((f.float(), [[], []]), (f.cpu(), [[], []]), (f[..., :2], [[], []]), (f, [[]])):
        with pytest.raises(ValueError):
            plot.draw_boxes_device(frames, boxes, None, boxes)
    with pytest.raises(ValueError):
        plot.draw_boxes_device(f, [[], []], None, [[], []], order="gbr")


def _batch_detect(yf, dev, decode, write, data_dir, out_dir, batch_size, in_flight):
    lines = []

    class H(logging.Handler):
        def emit(self, rec):
            lines.append(rec.getMessage())
    logger = logging.getLogger("yf-jpeg-write-%s-%s-%d-%d-%s" % (decode, write, batch_size, in_flight, os.path.basename(str(out_dir))))
    logger.setLevel(logging.INFO)
    logger.addHandler(H())
    logger.propagate = False
    io = yf.io_params_for(256)
    det = yf.Detect_YOLO(dev, os.path.join(WDIR, WEIGHTS[256]), {"io_params": io}, logger, decode=decode, write=write)
    det.batch_detect(str(data_dir), str(out_dir), batch_size=batch_size, in_flight=in_flight)
    return lines, det.last_labels


def _masked(lines):
    return [re.sub(r"\d+\.\d\dms", "<t>ms", x) for x in lines]


def _same_files(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names
    for name in names:
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    return names


def test_write_keyword_is_checked(yf, dev):
    with pytest.raises(ValueError, match="write must be"):
        yf.Detect_YOLO(dev, os.path.join(WDIR, WEIGHTS[256]), {"io_params": yf.io_params_for(256)}, logging.getLogger("w"), write="gpu")


@pytest.mark.parametrize("decode", ["host", "device"])
@pytest.mark.parametrize("batch_size,in_flight", [(8, 2), (8, 1), (256, 2)])
def test_batch_detect_device_write_writes_the_same_bytes(yf, dev, tmp_path, decode, batch_size, in_flight):
    (tmp_path / "host").mkdir()
    (tmp_path / "device").mkdir()
    lh, labels_h = _batch_detect(yf, dev, decode, "host", DATA, tmp_path / "host", batch_size, in_flight)
    ld, labels_d = _batch_detect(yf, dev, decode, "device", DATA, tmp_path / "device", batch_size, in_flight)
    assert len(lh) == 21 and _masked(lh) == _masked(ld)
    assert labels_h == labels_d and len(labels_d) == 20 and list(labels_h) == list(labels_d)
    assert len(_same_files(tmp_path / "host", tmp_path / "device")) == 20
    assert any(len(v) for v in labels_d.values())


@pytest.mark.parametrize("decode", ["host", "device"])
@pytest.mark.parametrize("batch_size,in_flight", [(8, 2), (256, 1)])
def test_batch_detect_device_write_with_two_frame_sizes(yf, dev, tmp_path, decode, batch_size, in_flight):
    data = tmp_path / "data"
    data.mkdir()
    names = sorted(os.listdir(DATA))
    for k, n in enumerate(names[:12]):
        if k % 3 == 1:                                   # every third frame at another size, so batches mix sizes
            Image.open(os.path.join(DATA, n)).convert("RGB").resize((328, 250)).save(data / n, quality=92)
        else:
            shutil.copy(os.path.join(DATA, n), data / n)
    (tmp_path / "host").mkdir()
    (tmp_path / "device").mkdir()
    lh, labels_h = _batch_detect(yf, dev, decode, "host", data, tmp_path / "host", batch_size, in_flight)
    ld, labels_d = _batch_detect(yf, dev, decode, "device", data, tmp_path / "device", batch_size, in_flight)
    assert len(lh) == 13 and _masked(lh) == _masked(ld) and labels_h == labels_d
    got = _same_files(tmp_path / "host", tmp_path / "device")
    assert {Image.open(tmp_path / "device" / n).size for n in got} == {(640, 512), (328, 250)}
