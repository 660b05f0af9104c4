"""Datasets from disk, host side: what the reference does before the first pixel is touched -- data yaml checks, the image file list,
label reading and verification, class filters, decoding and the rect-batch order (reference: ultralytics/data/utils.py:39-134,193-266,
data/base.py:97-140,211-234, data/dataset.py:30-131).  The rules are the reference's, pinned by tests/golden/g26_dataset.npz; the
code is this package's.  Pillow only (the reference verifies images with it too); cv2 is not needed.

Not reproduced (README "Out of scope"): `download:` of a data yaml (the key is ignored), restoring a JPEG without its end marker
(the pair is kept and a warning is logged: a dataset directory is never written to), the labels `*.cache` file, `.npy` image caches."""
import glob
import logging
import os
from multiprocessing.pool import ThreadPool
from pathlib import Path

import numpy as np

LOGGER = logging.getLogger("dedark_yolo_amd")
F32 = np.float32
IMG_FORMATS = ("bmp", "dng", "jpeg", "jpg", "mpo", "png", "tif", "tiff", "webp", "pfm")      # the reference's list (data/utils.py:27)
MAX_THREADS = 16
EXIF_ORIENTATION = 0x0112
_CLASSIFY = "the classify task reads one folder per class, not YOLO label files: pass loader="


def pool_size(workers=8):
    """threads of the verify / decode pools: the cfg's `workers`, at most 16, never the machine's CPU count"""
    return max(1, min(int(workers), MAX_THREADS))


# ---------------------------------------------------------------------------------------------------------------- data yaml
def _names_dict(names):
    """{index: name} from a list or a dict of names; the indices must be 0 .. n - 1"""
    pairs = enumerate(names) if isinstance(names, (list, tuple)) else names.items()
    out = {int(k): str(v) for k, v in pairs}
    if out and (min(out) < 0 or max(out) >= len(out)):
        raise KeyError(f"a {len(out)}-class dataset needs the class indices 0-{len(out) - 1}, the yaml has {min(out)}-{max(out)}")
    return out


def check_det_dataset(path):
    """The data yaml as a checked dict (reference check_det_dataset, data/utils.py:193-266, without any download):
      * `train` and `val` are required, and `names` or `nc`; both given must agree in length (SyntaxError, as the reference raises);
        a `names` list becomes {i: name}, missing names become class_i;
      * `path` that is not absolute is taken relative to the YAML FILE (the reference resolves it against the datasets directory of its
        settings file, which this package does not have); no `path` = the yaml's directory;
      * train / val / test -- a string or a list -- are resolved against it; a string that starts with '../' and does not exist is
        retried without it (the reference's rule);
      * every given split must exist: FileNotFoundError names the missing paths;
      * `download:` is ignored; kpt_shape, flip_idx and every other key pass through.
    Returns the dict with nc, names, path (a Path), the resolved splits and yaml_file."""
    import yaml
    file = Path(path)
    if not file.is_file():
        raise FileNotFoundError(f"data yaml '{path}' does not exist")
    with open(file, encoding="utf-8", errors="ignore") as f:
        data = yaml.safe_load(f) or {}
    absent = [k for k in ("train", "val") if k not in data]
    if absent:
        raise SyntaxError(f"{path}: '{absent[0]}:' is missing ('train' and 'val' are required in a data yaml)")
    has_names, has_nc = "names" in data, "nc" in data
    if not (has_names or has_nc):
        raise SyntaxError(f"{path}: neither 'names' nor 'nc' is given")
    if has_names and has_nc and len(data["names"]) != data["nc"]:
        raise SyntaxError(f"{path}: {len(data['names'])} names but nc: {data['nc']}")
    data["names"] = _names_dict(data["names"] if has_names else [f"class_{i}" for i in range(data["nc"])])
    data["nc"] = len(data["names"])
    data["yaml_file"] = str(file)
    root = Path(data.get("path") or file.parent)
    if not root.is_absolute():
        root = (file.parent / root).resolve()
    data["path"] = root

    def resolve(entry):
        return (root / entry).resolve()

    for split in ("train", "val", "test"):
        given = data.get(split)
        if not given:
            continue
        if isinstance(given, str):
            p = resolve(given)
            if not p.exists() and given.startswith("../"):
                p = resolve(given[3:])
            paths = data[split] = str(p)
            paths = [paths]
        else:
            paths = data[split] = [str(resolve(x)) for x in given]
        missing = [p for p in paths if not os.path.exists(p)]
        if missing:
            raise FileNotFoundError(f"{path}: the '{split}' split is not on disk: {missing}")
    return data


# ---------------------------------------------------------------------------------------------------------------- files
def get_img_files(img_path, fraction=1.0):
    """The image files of a split (reference BaseDataset.get_img_files, data/base.py:97-121): `img_path` is a directory (searched
    recursively), a text file with one image path per line (a leading './' stands for the list's own directory), or a list of either.
    Kept: files whose suffix is in IMG_FORMATS; sorted as strings; then the first round(n * fraction).  FileNotFoundError when an
    entry does not exist or nothing is left."""
    found = []
    for entry in (img_path if isinstance(img_path, (list, tuple)) else [img_path]):
        entry = Path(entry)
        if entry.is_dir():
            found.extend(glob.glob(str(entry / "**" / "*.*"), recursive=True))
        elif entry.is_file():
            here = str(entry.parent) + os.sep
            for line in entry.read_text().strip().splitlines():
                found.append(line.replace("./", here) if line.startswith("./") else line)
        else:
            raise FileNotFoundError(f"error loading data from {img_path}: {entry} does not exist")
    files = sorted(f.replace("/", os.sep) for f in found if f.split(".")[-1].lower() in IMG_FORMATS)
    if not files:
        raise FileNotFoundError(f"error loading data from {img_path}: no images found")
    return files[:round(len(files) * fraction)] if fraction < 1 else files


def img2label_paths(img_paths):
    """label file of every image (data/utils.py:39-42): the LAST '/images/' of the path becomes '/labels/', the suffix '.txt'"""
    a, b = f"{os.sep}images{os.sep}", f"{os.sep}labels{os.sep}"
    return [b.join(p.rsplit(a, 1)).rsplit(".", 1)[0] + ".txt" for p in img_paths]


# ---------------------------------------------------------------------------------------------------------------- labels
def _image_hw(im_file):
    """(h, w) as the label reader sees it, and the format: PIL verify; width and height swap for EXIF orientation 6 / 8 (the two the
    reference's exif_size knows, data/utils.py:53-60: only files PIL gives `_getexif` for, JPEG and its kin)"""
    from PIL import Image
    with Image.open(im_file) as im:
        im.verify()
        w, h = im.size
        try:
            if im._getexif().get(EXIF_ORIENTATION) in (6, 8):
                w, h = h, w
        except Exception:
            pass
        return (h, w), (im.format or "").lower()


def _polygon_boxes(segments):
    """xywh of the extent of every polygon (segments2boxes, utils/ops.py:516-530), float32"""
    ext = np.array([[s[:, 0].min(), s[:, 1].min(), s[:, 0].max(), s[:, 1].max()] for s in segments])
    out = np.empty_like(ext)
    out[:, 0], out[:, 1] = (ext[:, 0] + ext[:, 2]) / 2, (ext[:, 1] + ext[:, 3]) / 2
    out[:, 2], out[:, 3] = ext[:, 2] - ext[:, 0], ext[:, 3] - ext[:, 1]
    return out


def _check_rows(lb, keypoint, num_cls, width, ndim):
    """the reference's conditions on a non-empty label array (data/utils.py:95-108); ValueError names the first one that fails"""
    if lb.shape[1] != width:
        raise ValueError(f"{width} columns per label row expected, {lb.shape[1]} found")
    if keypoint:
        if not ((lb[:, 5::ndim] <= 1).all() and (lb[:, 6::ndim] <= 1).all()):
            raise ValueError("keypoint coordinates above 1 (not normalised)")
    else:
        if not (lb[:, 1:] <= 1).all():
            raise ValueError(f"coordinates above 1 (not normalised): {lb[:, 1:][lb[:, 1:] > 1]}")
        if not (lb >= 0).all():
            raise ValueError(f"negative label values: {lb[lb < 0]}")
    top = int(lb[:, 0].max())
    if not top <= num_cls:                                     # the reference's own `<=`: a class id equal to nc passes
        raise ValueError(f"class {top} in a dataset of {num_cls} classes (0-{num_cls - 1})")


def verify_image_label(args):
    """One (image, label file) pair: args = (im_file, lb_file, keypoint, num_cls, nkpt, ndim) ->
    (im_file, lb [n, 5] f32 (cls, normalised xywh), shape (h, w), segments, keypoints, missing, found, empty, corrupt, msg).
    The rules of the reference's verify_image_label (data/utils.py:63-134):
      * the image must verify, be at least 10 px on both sides and of a known format;
      * rows with more than 6 columns and no keypoints are polygons `cls x1 y1 x2 y2 ...`: `segments` gets the [k, 2] arrays, the
        boxes are the polygons' extents;
      * otherwise 5 columns; for pose 5 + nkpt * ndim, and with ndim == 2 a visibility column is appended to the keypoints: 0 where a
        coordinate is negative, else 1;
      * coordinates <= 1 (pose: keypoint x, y), no negative value (detect / segment), largest class <= num_cls;
      * duplicate rows are removed: the rows come back in np.unique(axis=0) order (first occurrences), the polygons with them;
      * a missing label file (missing = 1) or one without rows (empty = 1) gives zero labels.
    Any violation: the pair is dropped -- im_file None, corrupt = 1, msg says why.  A JPEG without its end marker is kept and a
    warning returned (the reference re-encodes and overwrites the file; not reproduced)."""
    im_file, lb_file, keypoint, num_cls, nkpt, ndim = args
    width = 5 + nkpt * ndim if keypoint else 5
    missing = found = empty = 0
    msg, segments = "", []
    try:
        shape, fmt = _image_hw(im_file)
        if min(shape) < 10:
            raise ValueError(f"image size {shape} is under 10 pixels")
        if fmt not in IMG_FORMATS:
            raise ValueError(f"image format '{fmt}' is not supported")
        if fmt in ("jpg", "jpeg"):
            with open(im_file, "rb") as f:
                f.seek(-2, os.SEEK_END)
                if f.read() != b"\xff\xd9":
                    msg = f"WARNING {im_file}: JPEG without end marker (corrupt?), used as it is"
        lb = np.zeros((0, width), dtype=F32)
        if not os.path.isfile(lb_file):
            missing = 1
        else:
            found = 1
            with open(lb_file) as f:
                rows = [line.split() for line in f.read().strip().splitlines() if line]
            if not keypoint and any(len(r) > 6 for r in rows):
                segments = [np.array(r[1:], dtype=F32).reshape(-1, 2) for r in rows]
                cls = np.array([r[0] for r in rows], dtype=F32).reshape(-1, 1)
                rows = np.concatenate((cls, _polygon_boxes(segments)), 1)
            rows = np.array(rows, dtype=F32)
            if len(rows) == 0:
                empty = 1
            else:
                _check_rows(rows, keypoint, num_cls, width, ndim)
                first = np.unique(rows, axis=0, return_index=True)[1]
                if len(first) < len(rows):
                    msg = f"WARNING {im_file}: {len(rows) - len(first)} duplicate labels removed"
                    rows = rows[first]
                    segments = [segments[i] for i in first] if segments else segments
                lb = rows
        keypoints = None
        if keypoint:
            keypoints = lb[:, 5:].reshape(-1, nkpt, ndim)
            if ndim == 2:
                vis = np.where((keypoints[..., 0] < 0) | (keypoints[..., 1] < 0), 0.0, 1.0).astype(F32)
                keypoints = np.concatenate([keypoints, vis[..., None]], axis=-1)
        return im_file, lb[:, :5], shape, segments, keypoints, missing, found, empty, 0, msg
    except Exception as e:
        return None, None, None, None, None, missing, found, empty, 1, f"WARNING {im_file}: image / label pair ignored: {e}"


def read_labels(im_files, task="detect", nc=80, kpt_shape=None, workers=8):
    """Labels of a list of image files (reference YOLODataset.cache_labels + get_labels, data/dataset.py:30-131, without the *.cache
    file): every pair goes through verify_image_label in a thread pool.  Returns (labels, (missing, found, empty, corrupt)) with
    labels[i] = dict(im_file, shape (h, w) EXIF-corrected, cls [n, 1] f32, bboxes [n, 4] f32 normalised xywh, segments, keypoints,
    normalized=True, bbox_format='xywh'), dropped pairs left out, in file order.  As in the reference:
      * no label file at all: a warning, then FileNotFoundError;
      * the set's polygon count differs from its box count (a detect / segment mix): a warning, and every `segments` is emptied;
      * all labels empty: ValueError;  a pose task without kpt_shape [K, 2 or 3]: ValueError."""
    if task == "classify":
        raise NotImplementedError(_CLASSIFY)
    keypoint = task == "pose"
    nkpt, ndim = (int(v) for v in (kpt_shape or (0, 0)))
    if keypoint and (nkpt <= 0 or ndim not in (2, 3)):
        raise ValueError("the data yaml's 'kpt_shape' is missing or wrong: [number of keypoints, 2 (x, y) or 3 (x, y, visible)]")
    lb_files = img2label_paths(im_files)
    labels, msgs, counts = [], [], np.zeros(4, dtype=np.int64)
    with ThreadPool(pool_size(workers)) as pool:
        jobs = [(im, lb, keypoint, int(nc), nkpt, ndim) for im, lb in zip(im_files, lb_files)]
        for im_file, lb, shape, segments, kp, *n, msg in pool.imap(verify_image_label, jobs):
            counts += n
            if im_file:
                labels.append(dict(im_file=im_file, shape=shape, cls=lb[:, 0:1], bboxes=lb[:, 1:], segments=segments, keypoints=kp,
                                   normalized=True, bbox_format="xywh"))
            if msg:
                msgs.append(msg)
    if msgs:
        LOGGER.info("\n".join(msgs))
    where = Path(lb_files[0]).parent if lb_files else ""
    missing, found, empty, corrupt = (int(v) for v in counts)
    if found == 0:
        LOGGER.warning(f"WARNING no labels found in {where}")
        raise FileNotFoundError(f"no labels found in {where}: cannot start without labels")
    n_cls, n_box, n_seg = (sum(len(lab[k]) for lab in labels) for k in ("cls", "bboxes", "segments"))
    if n_seg and n_seg != n_box:
        LOGGER.warning(f"WARNING {n_seg} polygons but {n_box} boxes in {where} (a detect / segment mix): only the boxes are used")
        for lab in labels:
            lab["segments"] = []
    if n_cls == 0:
        raise ValueError(f"all labels in {where} are empty: cannot start without labels")
    return labels, (missing, found, empty, corrupt)


def update_labels(labels, single_cls=False, classes=None):
    """the cfg's `classes` and `single_cls` (reference BaseDataset.update_labels, data/base.py:123-140), in place: rows of other
    classes are dropped together with their polygons / keypoints; single_cls then sets every class to 0"""
    wanted = None if classes is None else np.array(classes).reshape(1, -1)
    for lab in labels:
        if wanted is not None:
            keep = (lab["cls"] == wanted).any(1)
            lab["cls"], lab["bboxes"] = lab["cls"][keep], lab["bboxes"][keep]
            if lab["segments"]:
                lab["segments"] = [s for s, k in zip(lab["segments"], keep) if k]
            if lab["keypoints"] is not None:
                lab["keypoints"] = lab["keypoints"][keep]
        if single_cls:
            lab["cls"][:, 0] = 0
    return labels


def task_labels(labels, task):
    """the per-task view DeviceAugmentLoader / DeviceValLoader take: cls + bboxes, plus `segments` (segment) or `keypoints` (pose)"""
    if task == "classify":
        raise NotImplementedError(_CLASSIFY)
    extra = dict(detect=(), segment=("segments",), pose=("keypoints",))[task]
    return [{k: lab[k] for k in ("cls", "bboxes") + extra} for lab in labels]


def load_split(data, split, task, args):
    """files and labels of one split of a checked data dict: get_img_files (`fraction` for train only, as the reference's
    build_yolo_dataset passes it), read_labels, update_labels (single_cls, classes).  Returns (im_files, labels, counts)."""
    if not data.get(split):
        raise FileNotFoundError(f"the data yaml has no '{split}' split")
    fraction = float(getattr(args, "fraction", 1.0) or 1.0) if split == "train" else 1.0
    files = get_img_files(data[split], fraction)
    labels, counts = read_labels(files, task, data["nc"], data.get("kpt_shape"), getattr(args, "workers", 8))
    update_labels(labels, bool(getattr(args, "single_cls", False)), getattr(args, "classes", None))
    LOGGER.info(f"{split}: {counts[1]} labelled images, {counts[0] + counts[2]} backgrounds, {counts[3]} corrupt")
    return [lab["im_file"] for lab in labels], labels, counts


# ---------------------------------------------------------------------------------------------------------------- classify: folder datasets
# The classify task reads one folder per class (reference check_cls_dataset, data/utils.py:269-315, and torchvision's ImageFolder, which
# the reference's dataset class would wrap).  read_labels / task_labels / TaskLabels keep refusing "classify": these are its own entries.
CLS_IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")      # torchvision's IMG_EXTENSIONS


def check_cls_dataset(path, split=""):
    """A classification dataset directory as the reference's dict (check_cls_dataset, data/utils.py:269-315, without any download):
      train = <root>/train; val = <root>/val if it exists, else None; test likewise; the dict carries `val or test` under 'val' and
      `test or val` under 'test' (each falls back to the other); nc = number of directories under train/; names =
      dict(enumerate(sorted(directory names))).  `split` 'val' / 'test' that is not on disk only logs the fallback, as the reference.
    A missing root, or a root without train/, raises FileNotFoundError naming the path (the reference would try to download)."""
    root = Path(path)
    if not root.is_dir():
        raise FileNotFoundError(f"classify dataset '{path}' does not exist (expected a directory with train/ and val/ or test/)")
    root = root.resolve()
    train = root / "train"
    if not train.is_dir():
        raise FileNotFoundError(f"classify dataset '{root}' has no train/ directory: {train}")
    val = root / "val" if (root / "val").exists() else None
    test = root / "test" if (root / "test").exists() else None
    if split == "val" and not val:
        LOGGER.info("WARNING dataset 'split=val' not found, using 'split=test' instead.")
    elif split == "test" and not test:
        LOGGER.info("WARNING dataset 'split=test' not found, using 'split=val' instead.")
    names = sorted(x.name for x in train.iterdir() if x.is_dir())
    return dict(train=train, val=val or test, test=test or val, nc=len(names), names=dict(enumerate(names)))


def image_folder(root):
    """(files, cls, classes) of a directory with one sub-directory per class, by the rule of torchvision's ImageFolder (the package is
    absent; the rule is stated here):
      * classes = the sorted names of the sub-directories of `root`; class id = position in that list;
      * for each class in that order the tree below it is walked (links followed) with the directories and the file names of every
        directory sorted; a file is kept when its lower-cased name ends in one of CLS_IMG_EXTENSIONS;
      * no sub-directory at all, or a class without a kept file, raises FileNotFoundError naming the directory / the classes.
    files: list of str; cls: int64 [n]; classes: list of str."""
    root = str(root)
    if not os.path.isdir(root):
        raise FileNotFoundError(f"'{root}' is not a directory")
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"no class folders found in {root}")
    files, cls, empty = [], [], []
    for k, name in enumerate(classes):
        n0 = len(files)
        for d, dirs, fnames in os.walk(os.path.join(root, name), followlinks=True):
            dirs.sort()                                        # os.walk descends in the order the list is left in
            files += [os.path.join(d, f) for f in sorted(fnames) if f.lower().endswith(CLS_IMG_EXTENSIONS)]
        if len(files) == n0:
            empty.append(name)
        cls += [k] * (len(files) - n0)
    if empty:
        raise FileNotFoundError(f"no valid image file in class folder(s) {', '.join(empty)} of {root} "
                                f"(extensions: {', '.join(CLS_IMG_EXTENSIONS)})")
    return files, np.array(cls, dtype=np.int64), classes


def load_cls_split(data, split, args=None):
    """(files, cls) of one split of a check_cls_dataset dict.  `fraction` < 1 (cfg / args) keeps the first round(n * fraction) samples
    of the TRAINING split only.  A val / test split whose class folders are not exactly the training split's raises ValueError: the
    class id is the position in the split's own sorted folder list, so a missing or extra folder would shift the ids silently."""
    folder = data.get(split)
    if not folder:
        raise FileNotFoundError(f"the classify dataset has no '{split}' split")
    files, cls, classes = image_folder(folder)
    want = [data["names"][i] for i in range(len(data["names"]))]
    if split != "train" and classes != want:
        raise ValueError(f"{folder}: the class folders {classes} are not the training split's {want}: the class ids would not mean the same")
    if split == "train":
        fraction = float(getattr(args, "fraction", 1.0) or 1.0)
        if fraction < 1:
            n = round(len(files) * fraction)
            files, cls = files[:n], cls[:n]
    LOGGER.info(f"{split}: {len(files)} images in {len(classes)} classes")
    return files, cls


# ---------------------------------------------------------------------------------------------------------------- pixels
def decode(im_file):
    """uint8 HWC BGR (cv2.imread's layout, the one dy_aug_sample documents): PIL open -> EXIF transpose -> RGB -> channel flip.
    (cv2's JPEG decoder may differ from Pillow's by a level: unpinned.)"""
    from PIL import Image, ImageOps
    with Image.open(im_file) as im:
        rgb = np.asarray(ImageOps.exif_transpose(im).convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def decode_all(im_files, workers=8):
    """every file once, in order, in a pool of min(workers, 16) threads"""
    with ThreadPool(pool_size(workers)) as pool:
        return pool.map(decode, list(im_files))


# ---------------------------------------------------------------------------------------------------------------- rect batches
def set_rectangle(shapes, batch_size, imgsz, stride, pad):
    """Rect batching (reference BaseDataset.set_rectangle, data/base.py:211-234) for shapes [n, 2] = (h, w):
      order        [n]     images by ascending h / w -- numpy's DEFAULT argsort, ties as it leaves them (the same call, so the same order);
      batch_index  [n]     batch of every position of that order (floor(i / batch_size));
      batch_shapes [nb, 2] (H, W): a batch whose ratios are all below 1 is (max ratio, 1), all above 1 is (1, 1 / min ratio), else (1, 1);
                           times imgsz, up to the stride: ceil(x * imgsz / stride + pad) * stride."""
    hw = np.array(shapes)
    batch_index = np.floor(np.arange(len(hw)) / batch_size).astype(int)
    ratio = hw[:, 0] / hw[:, 1]
    order = ratio.argsort()
    ratio = ratio[order]
    unit = []
    for b in range(batch_index[-1] + 1):
        r = ratio[batch_index == b]
        lo, hi = r.min(), r.max()
        unit.append([hi, 1] if hi < 1 else [1, 1 / lo] if lo > 1 else [1, 1])
    batch_shapes = np.ceil(np.array(unit) * imgsz / stride + pad).astype(int) * stride
    return order, batch_index, batch_shapes
