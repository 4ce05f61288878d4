"""TEST INFRASTRUCTURE: the Pascal-VOC fixture trees of DetectDataset (dataset.py), assembled from committed data.

tests/golden/voc/xml/ holds one XML per frame: the 20 bundled frames of tests/golden/test_data/ (640x512 gray JPEGs; boxes from the
synthetic targets of golden_map_256.npz) and a few synthetic colour frames under tests/golden/voc/img/ (one at 600x800 for the
INTER_LINEAR path, one without objects, one with more than 64).  The JPEGs are linked, not copied:
    <root>/val/{img,xml}    the 20 bundled frames
    <root>/train/{img,xml}  the bundled frames and the synthetic ones"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
VOC = os.path.join(GOLDEN, "voc")
BUNDLED = os.path.join(GOLDEN, "test_data")
SYNTHETIC = ("syn_linear", "syn_empty", "syn_crowd")


def bundled_stems():
    return sorted(os.path.splitext(f)[0] for f in os.listdir(BUNDLED) if f.endswith(".jpg"))


def make_trees(root):
    """-> {"train": dir, "val": dir} under `root` (created), ready for aug_params' train_dataset_dir / val_dataset_dir."""
    out = {}
    for split, stems in (("val", bundled_stems()), ("train", bundled_stems() + list(SYNTHETIC))):
        d = os.path.join(str(root), split)
        os.makedirs(os.path.join(d, "img"), exist_ok=True)
        os.makedirs(os.path.join(d, "xml"), exist_ok=True)
        for s in stems:
            jpg = os.path.join(VOC, "img", s + ".jpg") if s in SYNTHETIC else os.path.join(BUNDLED, s + ".jpg")
            os.symlink(jpg, os.path.join(d, "img", s + ".jpg"))
            os.symlink(os.path.join(VOC, "xml", s + ".xml"), os.path.join(d, "xml", s + ".xml"))
        out[split] = d
    return out


def aug_params(trees, gussian_filter=0.6, fliplr=0.5):
    """The reference's augment_params keys (_config.py:23-36) over the fixture trees.  The blur probability is raised above the
    reference's 0.3 so that a few seeds reach every branch."""
    return {"train_dataset_dir": trees["train"], "val_dataset_dir": trees["val"], "degrees": 0.0, "translate": 0.0, "scale": 1.0,
            "shear": 0.0, "perspective": 0.0, "flipud": 0.0, "fliplr": fliplr, "mixup": 0.0, "gussian_filter": gussian_filter}
