"""`config_params` of the reference (src/model_training/_config.py): `io_params` (:2-20: anchors, shapes, thresholds, class names;
save_path / log_path relative instead of the author's home directory), `augment_params` (:23-36: the dataset directories, relative
like save_path, and the augmentation probabilities DetectDataset reads -- dataset.py) and `train_params` (:38-50), same names and meaning."""
import copy

config_params = {
    "io_params": {
        "save_path": "./models/",           # where train() writes YOLO-Fastest_epoch_N.pth
        "log_path": "./logs/",
        # three groups of three [w, h] anchors; heads use anchors[0], anchors[1] (detect.py:51).
        # 256x320 uses the first two groups, 512x640 the last two (_config.py:9).
        "anchors": [
            [[10, 13], [16, 30], [33, 23]],
            [[150, 75], [100, 100], [75, 150]],
            [[300, 150], [200, 200], [150, 300]],
        ],
        "input_channel": 1,
        "input_shape": [256, 320, 1],       # net input [rows, cols, channels], rows/cols multiples of 32
        "origin_img_shape": [512, 640, 3],  # dataset image [rows, cols, channels]
        "input_tensor_shape": (1, 1, 256, 320),
        "num_cls": 3,
        "num_anchors": 3,
        "anchor_mask": [[0, 1, 2], [3, 4, 5]],
        "strides": [16, 32],
        "conf_thre": 0.5,
        "nms_thre": 0.2,
        "class_names": ["carrier", "defender", "destroyer"],
    },
    "augment_params": {
        "train_dataset_dir": "./data/train_data/",   # Pascal-VOC trees: <dir>/xml/*.xml, <dir>/img/<stem>.jpg
        "val_dataset_dir": "./data/val_data/",
        "degrees": 0.0,                     # the reference does not implement these six (detect_dataset.py:131); DetectDataset does (dataset.py): neutral here
        "translate": 0.0,
        "scale": 1.0,
        "shear": 0.0,
        "perspective": 0.0,
        "flipud": 0.0,
        "fliplr": 0.5,                      # probability of a left-right flip
        "mixup": 0.0,
        "gussian_filter": 0.3,              # probability of a Gaussian blur (then 7x7 with probability 0.4, else 3x3); the reference's spelling
    },
    "train_params": {
        "pretrained_pth": "",               # a .pth to start from; otherwise initialize_weights()
        "total_epochs": 30,
        "batch_size": 16,
        "lr0": 0.001,                       # initial learning rate (Adam)
        "momentum": 0.937,                  # SGD momentum / Adam beta1 (yolov5's hyp key): read by training.train(optimizer="sgd" | "adam") only; the reference's Adam call (train.py:84) passes betas explicitly
        "weight_decay": 0.0005,             # on the convolution weights: read by training.train(optimizer="sgd" | "adam") only; the reference passes none (train.py:84)
        "branch_weight": [1.0, 1.0],        # per-head loss factors: read by training.train(branch_weight=True) only; the reference sums the heads unweighted (train.py:129-130)
        "IOU_loss_thre": 0.5,               # anchors whose shape IoU with a target exceeds this are not punished as background
        "IOU_val_thre": 0.5,                # match threshold of the mAP computation
    },
}


def io_params_for(rows):
    """io_params for the two shipped checkpoints: rows=256 (256x320) or rows=512 (512x640, anchor groups 1..2,
    no resize)."""
    io = copy.deepcopy(config_params["io_params"])
    if rows == 512:
        io["input_shape"] = [512, 640, 1]
        io["input_tensor_shape"] = (1, 1, 512, 640)
        io["anchors"] = io["anchors"][1:]
    elif rows != 256:
        raise ValueError("shipped checkpoints are 256x320 and 512x640")
    return io
