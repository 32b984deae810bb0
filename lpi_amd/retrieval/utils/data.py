"""Dataset I/O contract of the retrieval path (utils/data.py:160-382 of the reference): train items are
``(image[3,224,224] f32 ImageNet-normalised, caption, 0, task)``, eval items ``(image, img_id, task)`` with the lookup tables
``text, image, text_cat, txt2img, img2txt`` on the dataset object.  COCO itself is not available offline, so the default
implementation is synthetic (captions are delivered as ready token ids).  ``Coco`` / ``CocoEval`` read the reference's annotation
format (a JSON list of ``{"image", "caption", "category", "image_id"}`` records, ``caption`` a string for training and a list for
evaluation) from ``image_root`` / ``ann_file`` with PIL — the torchvision pipelines of the reference (RandomResizedCrop +
RandomHorizontalFlip / Resize(256) + CenterCrop(224), ToTensor, ImageNet Normalize) are restated here on PIL + torch, because
torchvision is not part of this environment.  Host-side I/O only: nothing here is on the timed path."""
import json
import math
import os
import re

import numpy as np
import torch
from torch.utils.data import Dataset

from lpi_amd import synth


def pre_caption(caption, max_words):
    """utils/data.py:160-185."""
    caption = re.sub(r"([,.'!?\"()*#:;~])", '', caption.lower()).replace('-', ' ').replace('/', ' ').replace('<person>', 'person')
    caption = re.sub(r"\s{2,}", ' ', caption).rstrip('\n').strip(' ')
    words = caption.split(' ')
    if len(words) > max_words:
        caption = ' '.join(words[:max_words])
    if not len(caption):
        raise ValueError("pre_caption yields invalid text")
    return caption


class SyntheticCoco(Dataset):
    """Training pairs of one task: N(0,1) images and random captions (SURVEY.md section 8(d) recipe).

    captions = 'ids' (default): a caption is its row of ready token ids [77] (no tokenizer, no merge table needed); 'strings': a caption is a STRING of
    COCO-like words (lpi_amd.synth_bpe.captions) — the item then has exactly the reference's structure (utils/data.py:376-382: f32 image, str, 0, task) and
    the step tokenises it like PromptLearner.forward does.
    pixel_format = 'u8': items carry uint8 CHW pixels (uniform bytes) and ToTensor + Normalize run on the GPU (lpi_patchify_u8).
    pixel_format = 'decoded': items carry a DecodedImage: seeded uniform-byte HWC images of random size (64..900 px a side) and train_crop_params for a
    `resolution` output (the crop / resize / flip then run on the GPU: lpi_amd.imageops).
    image_pool = K > 0: the K distinct images are generated once and item i returns pool image i % K (a VIEW: the collate / pipeline copies it) — an
    item costs nothing, so that a throughput measurement of the training loop times the loop and not numpy's generator (150 k normals per image)."""

    def __init__(self, n, tasks, resolution=224, seed=0, captions="ids", image_pool=0, pixel_format="f32"):
        if captions not in ("ids", "strings"):
            raise ValueError(f"captions must be 'ids' or 'strings', not {captions!r}")
        _check_pixel_format(pixel_format)
        if pixel_format == "jpeg":
            raise ValueError("pixel_format='jpeg' needs image files: SyntheticCoco has none (use 'decoded')")
        self.pixel_format = pixel_format
        self.n, self.tasks, self.res = n, list(tasks), resolution
        self.seed = seed
        if captions == "ids":
            self.ids = torch.from_numpy(synth.token_ids(n, seed=synth.TOKEN_SEED + 17 * seed))
            self.captions = None
        else:
            from lpi_amd.synth_bpe import captions as make
            self.ids, self.captions = None, make(n, seed=synth.TOKEN_SEED + 17 * seed)
        k = min(int(image_pool), n) if image_pool else 0
        if pixel_format == "decoded":     # image i: its own seeded size and bytes (image i % K of a pool of K, made once)
            self.pool = [self._decoded(j) for j in range(k)] if k else None
        elif pixel_format == "u8":          # uniform bytes: "decoded pixels"; pixel_format='f32' of the same dataset = their ToTensor + Normalize
            k = k or n
            self.pool = torch.from_numpy(synth._rng(synth.IMAGE_SEED + seed, f"u8pool{k}").integers(0, 256, (k, 3, resolution, resolution), dtype=np.uint8))
        else:
            self.pool = None if k <= 0 else torch.from_numpy(synth.normal(synth.IMAGE_SEED + seed, f"pool{k}", (k, 3, resolution, resolution)))

    def __len__(self):
        return self.n

    def _decoded(self, j):
        rng = synth._rng(synth.IMAGE_SEED + self.seed, f"decoded{j}")
        w, h = (int(v) for v in rng.integers(64, 901, 2))
        return torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))

    def __getitem__(self, i):
        if self.pixel_format == "decoded":
            px = self.pool[i % len(self.pool)] if self.pool is not None else self._decoded(i)
            img = DecodedImage(px, train_crop_params(int(px.shape[1]), int(px.shape[0]), self.res), self.res)
        elif self.pool is not None:
            img = self.pool[i % self.pool.shape[0]]
        else:
            img = torch.from_numpy(synth.normal(synth.IMAGE_SEED + self.seed, f"img{i}", (3, self.res, self.res)))
        return img, (self.ids[i] if self.captions is None else self.captions[i]), 0, self.tasks[0]


def collate_keep_images(batch):
    """default_collate for everything but the images, which stay a LIST of [3,R,R] tensors: lpi_amd.pipeline gathers them straight into its pinned staging
    buffer (one copy, several threads) instead of torch.stack into pageable memory followed by a second copy (single-process loaders only: tensors that
    cross a worker boundary must be stacked there)."""
    from torch.utils.data import default_collate
    cols = list(zip(*batch))
    return [list(cols[0])] + [default_collate(list(c)) for c in cols[1:]]


INTERPOLATIONS = ("bilinear", "bicubic", "box")      # the Pillow filters lpi_image_resample_u8_f restates (lpi_amd.imageops.FILTERS)


def _check_filter(filter):
    if filter not in INTERPOLATIONS:
        raise ValueError(f"interpolation must be 'bilinear', 'bicubic' or 'box', not {filter!r}")
    return filter


def _common_filter(imgs, who):
    filter = imgs[0].filter
    if any(d.filter != filter for d in imgs):
        raise ValueError(f"{who}: the items of one batch must share the resampling filter (the kernel takes one per call)")
    return filter


def _rebuild(cls, filter, *args):
    """Unpickles an image / batch class whose filter is a keyword argument."""
    return cls(*args, filter=filter)


def _rebuild_encoded(cls, filter, progressive, layouts, *args):
    """Unpickles EncodedImage / EncodedBatch: filter, progressive and layouts are keyword arguments."""
    return cls(*args, filter=filter, progressive=progressive, layouts=layouts)


class DecodedImage:
    """An item's image in pixel_format='decoded': the decoded RGB pixels at their original size (``pixels``: HWC uint8, np.array(img.convert("RGB"))
    as a tensor, not copied to CHW) and the transform's geometry (``params``: the DESCRIPTOR_FIELDS tuple of train_crop_params / test_crop_params)
    for an S x S output (``size``) with the resampling filter ``filter`` ('bilinear' | 'bicubic' | 'box').  lpi_amd.imageops.resample_decoded runs
    the crop / resize / flip on the GPU."""
    __slots__ = ("pixels", "params", "size", "filter")

    def __init__(self, pixels, params, size, *, filter="bilinear"):
        if not torch.is_tensor(pixels) or pixels.dtype != torch.uint8 or pixels.dim() != 3 or pixels.shape[2] != 3:
            raise ValueError("DecodedImage.pixels must be an HWC uint8 tensor with 3 channels")
        h, w = int(pixels.shape[0]), int(pixels.shape[1])
        self.pixels, self.size, self.filter = pixels, int(size), _check_filter(filter)
        x0, y0, x1, y1, rw, rh, ox, oy, flip = params
        self.params = resample_descriptor(w, h, (x0, y0, x1, y1), (rw, rh), (ox, oy), flip, size)

    def __reduce__(self):
        return (_rebuild, (DecodedImage, self.filter, self.pixels, self.params, self.size))


class DecodedBatch:
    """A batch of DecodedImage: ``pixels`` a list of B HWC uint8 tensors (ragged), ``params`` the [B, 9] int64 descriptor table, ``size`` S,
    ``filter`` the one resampling filter of the batch (the kernel takes it per call)."""
    __slots__ = ("pixels", "params", "size", "filter")

    def __init__(self, pixels, params, size, *, filter="bilinear"):
        self.pixels, self.params, self.size, self.filter = list(pixels), params, int(size), _check_filter(filter)

    def __len__(self):
        return len(self.pixels)

    def __reduce__(self):
        return (_rebuild, (DecodedBatch, self.filter, self.pixels, self.params, self.size))

    def pin_memory(self, device=None):
        return DecodedBatch([p.pin_memory() for p in self.pixels], self.params.pin_memory(), self.size, filter=self.filter)


def collate_decoded(batch):
    """Collate of pixel_format='decoded' items ``(DecodedImage, ...)``: the images become one DecodedBatch (no pixel is copied), every other field goes
    through default_collate.  Works in worker processes (the batch pickles, its tensors travel in shared memory) and with pin_memory=True."""
    from torch.utils.data import default_collate
    cols = list(zip(*batch))
    imgs = cols[0]
    if not all(isinstance(d, DecodedImage) for d in imgs):
        raise ValueError("collate_decoded takes items whose first field is a DecodedImage (pixel_format='decoded')")
    size = imgs[0].size
    if any(d.size != size for d in imgs):
        raise ValueError("collate_decoded: the items of one batch must share the output size S")
    filter = _common_filter(imgs, "collate_decoded")
    params = torch.tensor([d.params for d in imgs], dtype=torch.int64).view(len(imgs), len(DESCRIPTOR_FIELDS))
    return [DecodedBatch([d.pixels for d in imgs], params, size, filter=filter)] + [default_collate(list(c)) for c in cols[1:]]


class EncodedImage:
    """An item's image in pixel_format='jpeg': the file's bytes still compressed (``data``: a uint8 tensor), the transform's geometry (``params``: the
    DESCRIPTOR_FIELDS tuple of train_crop_params / test_crop_params of the frame size), the output size S (``size``), the frame size (``wh``) and
    the resampling filter (``filter``: 'bilinear' | 'bicubic' | 'box').
    The file is inside lpi_jpeg_decode_u8's envelope (lpi_amd.imageops.jpeg_info) or, with ``progressive`` = True, inside the wider one of
    LPI_JPEG_PROGRESSIVE and, with ``layouts`` = True, of LPI_JPEG_LAYOUTS (lpi_jpeg_decode_u8_x); lpi_amd.imageops.resample_encoded decodes and
    resamples it on the GPU."""
    __slots__ = ("data", "params", "size", "wh", "filter", "progressive", "layouts")

    def __init__(self, data, params, size, wh, *, filter="bilinear", progressive=False, layouts=False):
        self.progressive, self.layouts = bool(progressive), bool(layouts)
        if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError("EncodedImage.data must be a 1-D uint8 tensor (the file's bytes)")
        w, h = (int(v) for v in wh)
        self.data, self.size, self.wh, self.filter = data, int(size), (w, h), _check_filter(filter)
        x0, y0, x1, y1, rw, rh, ox, oy, flip = params
        self.params = resample_descriptor(w, h, (x0, y0, x1, y1), (rw, rh), (ox, oy), flip, size)

    def __reduce__(self):
        return (_rebuild_encoded, (EncodedImage, self.filter, self.progressive, self.layouts, self.data, self.params, self.size, self.wh))


class EncodedBatch:
    """A batch of pixel_format='jpeg' items: ``data`` ONE uint8 tensor with the files of the encoded items back to back (file i = data[offsets[i] :
    offsets[i+1]], empty for a host-decoded item), ``offsets`` [B+1] int64, ``params`` the [B, 9] int64 descriptor table, ``wh`` [B, 2] int64 frame
    sizes, ``size`` S, ``fallback`` {batch index: HWC uint8 pixels} of the items Pillow decoded in the worker (files outside the envelope),
    ``filter`` the one resampling filter of the batch, ``progressive`` whether its files were admitted by the envelope of LPI_JPEG_PROGRESSIVE (the
    decode then goes through lpi_jpeg_decode_u8_x with that flag), ``layouts`` the same for LPI_JPEG_LAYOUTS."""
    __slots__ = ("data", "offsets", "params", "wh", "size", "fallback", "filter", "progressive", "layouts")

    def __init__(self, data, offsets, params, wh, size, fallback=None, *, filter="bilinear", progressive=False, layouts=False):
        self.data, self.offsets, self.params, self.wh, self.size = data, offsets, params, wh, int(size)
        self.progressive, self.layouts = bool(progressive), bool(layouts)
        self.fallback = dict(fallback or {})
        self.filter = _check_filter(filter)

    def __len__(self):
        return int(self.params.shape[0])

    def file(self, i):
        """File i's bytes (a uint8 tensor view)."""
        return self.data[int(self.offsets[i]):int(self.offsets[i + 1])]

    def __reduce__(self):
        return (_rebuild_encoded, (EncodedBatch, self.filter, self.progressive, self.layouts, self.data, self.offsets, self.params, self.wh, self.size,
                                   self.fallback))

    def pin_memory(self, device=None):
        return EncodedBatch(self.data.pin_memory(), self.offsets, self.params, self.wh, self.size, {i: p.pin_memory() for i, p in self.fallback.items()},
                            filter=self.filter, progressive=self.progressive, layouts=self.layouts)


def collate_encoded(batch):
    """Collate of pixel_format='jpeg' items ``(EncodedImage or DecodedImage, ...)``: the images become one EncodedBatch whose file bytes are packed into
    a single tensor here (in the worker: one shared-memory tensor per batch), every other field goes through default_collate."""
    from torch.utils.data import default_collate
    cols = list(zip(*batch))
    imgs = cols[0]
    if not all(isinstance(d, (EncodedImage, DecodedImage)) for d in imgs):
        raise ValueError("collate_encoded takes items whose first field is an EncodedImage or a DecodedImage (pixel_format='jpeg')")
    size = imgs[0].size
    if any(d.size != size for d in imgs):
        raise ValueError("collate_encoded: the items of one batch must share the output size S")
    filter = _common_filter(imgs, "collate_encoded")
    n = [int(d.data.numel()) if isinstance(d, EncodedImage) else 0 for d in imgs]
    offsets = torch.tensor([0] + n, dtype=torch.int64).cumsum(0)
    data = torch.empty(int(offsets[-1]), dtype=torch.uint8)
    fallback, wh = {}, []
    for i, d in enumerate(imgs):
        if isinstance(d, EncodedImage):
            data[int(offsets[i]):int(offsets[i + 1])] = d.data
            wh.append(d.wh)
        else:
            fallback[i] = d.pixels
            wh.append((int(d.pixels.shape[1]), int(d.pixels.shape[0])))
    params = torch.tensor([d.params for d in imgs], dtype=torch.int64).view(len(imgs), len(DESCRIPTOR_FIELDS))
    progressive = any(isinstance(d, EncodedImage) and d.progressive for d in imgs)
    layouts = {d.layouts for d in imgs if isinstance(d, EncodedImage)}
    if len(layouts) > 1:
        raise ValueError("collate_encoded: the items of one batch must share the layouts setting (the envelope their files were admitted by)")
    return [EncodedBatch(data, offsets, params, torch.tensor(wh, dtype=torch.int64).view(len(imgs), 2), size, fallback, filter=filter,
                         progressive=progressive, layouts=True in layouts)] + \
        [default_collate(list(c)) for c in cols[1:]]


PIXEL_FORMATS = ("f32", "u8", "decoded", "jpeg")


def _check_pixel_format(pixel_format):
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError(f"pixel_format must be 'f32', 'u8', 'decoded' or 'jpeg', not {pixel_format!r}")


class SyntheticCocoEval(Dataset):
    """Eval set over tasks 0..t: n_img images per task, `cpi` captions per image."""

    def __init__(self, n_img_per_task, tasks, cpi=2, resolution=224, seed=1):
        self.res, self.seed = resolution, seed
        self.image, self.text, self.text_cat, self.img_cat = [], [], [], []
        self.txt2img, self.img2txt = {}, {}
        for t in tasks:
            for _ in range(n_img_per_task):
                i = len(self.image)
                self.image.append(i)
                self.img_cat.append(int(t))
                self.img2txt[i] = []
                for _ in range(cpi):
                    j = len(self.text)
                    self.text.append(j)
                    self.text_cat.append(int(t))
                    self.txt2img[j] = i
                    self.img2txt[i].append(j)
        self.ids = torch.from_numpy(synth.token_ids(len(self.text), seed=synth.TOKEN_SEED + 1000 + seed))
        self.text = self.ids          # "texts" are token-id rows; slicing works like the reference's list slicing

    def __len__(self):
        return len(self.image)

    def __getitem__(self, i):
        img = torch.from_numpy(synth.normal(synth.IMAGE_SEED + 500 + self.seed, f"img{i}", (3, self.res, self.res)))
        return img, i, self.img_cat[i]


# ---------------------------------------------------------------------------------------------- real COCO (utils/data.py:186-382)
# task t of the 12-task protocol holds COCO super-category TASK_CATEGORIES[t] (utils/data.py:233-249, 338-353)
TASK_CATEGORIES = (11, 6, 3, 10, 5, 12, 7, 9, 2, 8, 4, 1)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# CLIP's own statistics (models/clip/clip.py:77 of the reference)
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
NORMALIZATIONS = {"imagenet": (IMAGENET_MEAN, IMAGENET_STD), "clip": (CLIP_MEAN, CLIP_STD)}


def norm_stats(normalize):
    """(mean, std) of a normalisation: 'imagenet', 'clip', or a (mean, std) pair of three floats each."""
    if isinstance(normalize, str):
        if normalize not in NORMALIZATIONS:
            raise ValueError(f"normalize must be 'imagenet', 'clip' or a (mean, std) pair, not {normalize!r}")
        return NORMALIZATIONS[normalize]
    try:
        mean, std = normalize
        mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    except (TypeError, ValueError):
        raise ValueError(f"normalize must be 'imagenet', 'clip' or a (mean, std) pair, not {normalize!r}") from None
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("a (mean, std) pair holds three values each")
    return mean, std


def task_of_category(category: int) -> int:
    """The reference's loop `for z in range(len(tasks)): if category in tasks[z]: new_category = z` (0 when absent)."""
    return TASK_CATEGORIES.index(category) if category in TASK_CATEGORIES else 0


def _pil():
    try:
        from PIL import Image
    except ImportError as e:          # loud: there is no silent fallback to synthetic data
        raise ImportError("the COCO datasets need Pillow (PIL) to decode images; use dataset_impl='synthetic' without it") from e
    return Image


def _to_u8_chw(img):
    """The decoded pixels as the GPU takes them (pixel_format='u8'): HWC uint8 -> CHW uint8; ToTensor + Normalize then run inside lpi_patchify_u8."""
    return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).contiguous()


def normalise_u8(u8, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """ToTensor + Normalize on a CHW (or BCHW) uint8 tensor, in the operations of _to_normalised_tensor — the f32 image the 'f32' pixel format delivers."""
    a = u8.float().div_(255.0)
    shape = (3, 1, 1)
    return (a - torch.tensor(mean).view(shape)) / torch.tensor(std).view(shape)


def _to_normalised_tensor(img, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """ToTensor + Normalize (utils/data.py:201-204; ImageNet statistics by default): HWC uint8 -> CHW f32 in [0,1], then (x - mean) / std."""
    a = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div_(255.0)
    mean = torch.tensor(mean).view(3, 1, 1)
    std = torch.tensor(std).view(3, 1, 1)
    return (a - mean) / std


def train_crop_params(w, h, size=224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """The random draws of train_transform (RandomResizedCrop + RandomHorizontalFlip, torch RNG, in this order): a crop of random area (scale x image
    area) and log-uniform aspect ratio, ten attempts, else the largest centred crop inside the ratio bounds; then the flip's torch.rand(1).
    Returns the descriptor of the image (see resample_descriptor): crop box, resized to (size, size), window at (0, 0), flip flag."""
    area = w * h
    box = None
    for _ in range(10):
        target = area * float(torch.empty(1).uniform_(scale[0], scale[1]))
        logr = float(torch.empty(1).uniform_(math.log(ratio[0]), math.log(ratio[1])))
        ar = math.exp(logr)
        cw, ch = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
        if 0 < cw <= w and 0 < ch <= h:
            top = int(torch.randint(0, h - ch + 1, (1,)))
            left = int(torch.randint(0, w - cw + 1, (1,)))
            box = (left, top, left + cw, top + ch)
            break
    if box is None:
        in_ratio = w / h
        if in_ratio < ratio[0]:
            cw, ch = w, int(round(w / ratio[0]))
        elif in_ratio > ratio[1]:
            cw, ch = int(round(h * ratio[1])), h
        else:
            cw, ch = w, h
        left, top = (w - cw) // 2, (h - ch) // 2
        box = (left, top, left + cw, top + ch)
    flip = float(torch.rand(1)) < 0.5
    return resample_descriptor(w, h, box, (size, size), (0, 0), flip, size)


def test_crop_params(w, h, resize=256, size=224):
    """The geometry of test_transform (Resize(resize) of the shorter side + CenterCrop(size)): the whole image resized to (nw, nh), the window at the
    centre-crop origin, no flip.  No random draws."""
    if w <= h:
        nw, nh = resize, int(resize * h / w)
    else:
        nw, nh = int(resize * w / h), resize
    left, top = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))
    return resample_descriptor(w, h, (0, 0, w, h), (nw, nh), (left, top), False, size)


# one image's geometry, the row of a DecodedBatch's descriptor table: crop(box).resize((rw, rh), the batch's filter), the window [ox, ox+S) x [oy, oy+S), mirrored if flip
DESCRIPTOR_FIELDS = ("x0", "y0", "x1", "y1", "rw", "rh", "ox", "oy", "flip")


def resample_descriptor(w, h, box, resized, origin, flip, size):
    """Validated descriptor tuple (DESCRIPTOR_FIELDS) of a w x h image; ValueError when the box leaves the image, a size is not positive, or the S x S
    window leaves the resized image."""
    x0, y0, x1, y1 = (int(v) for v in box)
    rw, rh = (int(v) for v in resized)
    ox, oy = (int(v) for v in origin)
    size, w, h = int(size), int(w), int(h)
    if w < 1 or h < 1:
        raise ValueError(f"image size must be positive, not {w} x {h}")
    if size < 1:
        raise ValueError(f"output size S must be >= 1, not {size}")
    if not (0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h):
        raise ValueError(f"crop box {(x0, y0, x1, y1)} is empty or leaves the {w} x {h} image")
    if rw < 1 or rh < 1:
        raise ValueError(f"resized size must be positive, not {rw} x {rh}")
    if not (0 <= ox and ox + size <= rw and 0 <= oy and oy + size <= rh):
        raise ValueError(f"the {size} x {size} window at {(ox, oy)} leaves the {rw} x {rh} resized image")
    return (x0, y0, x1, y1, rw, rh, ox, oy, int(bool(flip)))


def _pil_filter(interpolation):
    Image = _pil()
    return {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "box": Image.BOX}[_check_filter(interpolation)]


def apply_descriptor(img, desc, size, interpolation="bilinear"):
    """The descriptor applied with Pillow: the PIL image the transforms produce (the GPU kernel lpi_image_resample_u8_f reproduces it byte for byte)."""
    Image = _pil()
    x0, y0, x1, y1, rw, rh, ox, oy, flip = desc
    img = img.crop((x0, y0, x1, y1)).resize((rw, rh), _pil_filter(interpolation))
    if (ox, oy, rw, rh) != (0, 0, size, size):
        img = img.crop((ox, oy, ox + size, oy + size))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return img


def train_transform(img, size=224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), pixel_format="f32", interpolation="bilinear", normalize="imagenet"):
    """RandomResizedCrop(size) + RandomHorizontalFlip + ToTensor + Normalize (utils/data.py:193-204), torch RNG (train_crop_params); bilinear and
    ImageNet statistics unless told otherwise."""
    w, h = img.size
    img = apply_descriptor(img, train_crop_params(w, h, size, scale, ratio), size, interpolation)
    return _to_u8_chw(img) if pixel_format == "u8" else _to_normalised_tensor(img, *norm_stats(normalize))


def test_transform(img, resize=256, size=224, pixel_format="f32", interpolation="bilinear", normalize="imagenet"):
    """Resize(256) (shorter side, bilinear) + CenterCrop(224) + ToTensor + Normalize (utils/data.py:197-204; test_crop_params).  CLIP's own
    preprocessing (models/clip/clip.py:71-78) is resize == size, interpolation='bicubic', normalize='clip'."""
    w, h = img.size
    img = apply_descriptor(img, test_crop_params(w, h, resize, size), size, interpolation)
    return _to_u8_chw(img) if pixel_format == "u8" else _to_normalised_tensor(img, *norm_stats(normalize))


def _load(image_root, name, transform):
    Image = _pil()
    with Image.open(os.path.join(image_root, name)) as im:
        return transform(im.convert("RGB"))


def decoded_transform(form, size=224, resize=256, interpolation="bilinear"):
    """The transform of pixel_format='decoded': PIL image -> DecodedImage(HWC pixels, descriptor of form 'train' (train_crop_params: the random draws
    happen here, in the order of train_transform) or 'center' (test_crop_params))."""
    if form not in ("train", "center"):
        raise ValueError(f"form must be 'train' or 'center', not {form!r}")
    _check_filter(interpolation)

    def transform(img):
        w, h = img.size
        desc = train_crop_params(w, h, size) if form == "train" else test_crop_params(w, h, resize, size)
        # np.asarray of a PIL image is a read-only view of a bytes object: np.array takes a writable copy (0.1 ms for 640 x 480)
        return DecodedImage(torch.from_numpy(np.array(img if img.mode == "RGB" else img.convert("RGB"), dtype=np.uint8)), desc, size,
                            filter=interpolation)
    return transform


def encoded_transform(form, size=224, resize=256, interpolation="bilinear", progressive=False, layouts=False):
    """The transform of pixel_format='jpeg': file bytes -> EncodedImage (inside the envelope; lpi_jpeg_info gives the frame size, host only) or, for
    any other file, Pillow's decode as a DecodedImage, right here (decoded_transform).  The crop draws are decoded_transform's, in its order.
    progressive: the envelope of LPI_JPEG_PROGRESSIVE (progressive files with a complete scan script are the GPU's too); layouts: that of
    LPI_JPEG_LAYOUTS (baseline 4:4:0, 4:1:1, 1x4, RGB, CMYK and YCCK files are the GPU's too)."""
    fallback = decoded_transform(form, size, resize, interpolation)
    progressive, layouts = bool(progressive), bool(layouts)

    def transform(data):
        from lpi_amd.imageops import jpeg_info
        info = jpeg_info(data, progressive=progressive, layouts=layouts)
        if info is None or not info[0]:
            import io
            Image = _pil()
            with Image.open(io.BytesIO(data)) as im:
                return fallback(im.convert("RGB"))
        _, w, h = info
        desc = train_crop_params(w, h, size) if form == "train" else test_crop_params(w, h, resize, size)
        return EncodedImage(torch.frombuffer(bytearray(data), dtype=torch.uint8), desc, size, (w, h), filter=interpolation, progressive=progressive,
                            layouts=layouts)
    return transform


def _check_jpeg_progressive(jpeg_progressive, pixel_format):
    if jpeg_progressive and pixel_format != "jpeg":
        raise ValueError(f"jpeg_progressive widens the envelope of pixel_format='jpeg': it cannot go with pixel_format={pixel_format!r}")
    return bool(jpeg_progressive)


def _check_jpeg_layouts(jpeg_layouts, pixel_format):
    if jpeg_layouts and pixel_format != "jpeg":
        raise ValueError(f"jpeg_layouts widens the envelope of pixel_format='jpeg': it cannot go with pixel_format={pixel_format!r}")
    return bool(jpeg_layouts)


PREPROCESS = ("reference", "clip")


def preprocess_options(args, resolution=None):
    """The image preprocessing a config asks for, as {'interpolation', 'normalize', 'eval_resize', 'size'} (None when the config names none of the keys:
    the datasets and the engine are then built exactly as without them).  Config keys: `preprocess` = 'reference' (default: the reference's retrieval
    loader — bilinear, ImageNet statistics, Resize(256) for evaluation, 224 x 224 items) or 'clip' (CLIP's own, models/clip/clip.py:71-78 of the
    reference: bicubic, CLIP's statistics, Resize(n_px) + CenterCrop(n_px) for evaluation, n_px = `resolution`, the model's); `interpolation`
    ('bilinear' | 'bicubic' | 'box'), `normalize` ('imagenet' | 'clip' | a (mean, std) pair) and `eval_resize` override single parts of it.
    `image_resolution` (the model run at another input resolution than its checkpoint's, models/slinet.py model_resolution) counts as one of the keys, and only
    with it does 'reference' leave its 224 / 256: the items are image_resolution x image_resolution and evaluation resizes to
    round(image_resolution * 256 / 224) first — the loader's own ratio — unless `eval_resize` says otherwise.  'clip' follows `resolution` as ever."""
    keys = ("preprocess", "interpolation", "normalize", "eval_resize")
    if not any(k in args for k in keys + ("image_resolution",)):
        return None
    pre = args.get("preprocess", "reference")
    if pre not in PREPROCESS:
        raise ValueError(f"preprocess must be 'reference' or 'clip', not {pre!r}")
    if pre == "clip":
        if resolution is None:
            raise ValueError("preprocess='clip' needs the model's image resolution")
        out = {"interpolation": "bicubic", "normalize": "clip", "eval_resize": int(resolution), "size": int(resolution)}
    else:
        out = {"interpolation": "bilinear", "normalize": "imagenet", "eval_resize": 256, "size": 224}
        if "image_resolution" in args:
            r = args["image_resolution"]
            if isinstance(r, bool) or not isinstance(r, int) or r <= 0:
                raise ValueError(f"image_resolution must be a positive integer, not {r!r}")
            out.update(size=r, eval_resize=int(round(r * 256 / 224)))
    for k in keys[1:]:
        if k in args:
            out[k] = args[k]
    _check_filter(out["interpolation"])
    norm_stats(out["normalize"])
    out["eval_resize"] = int(out["eval_resize"])
    if out["eval_resize"] < out["size"]:
        raise ValueError(f"eval_resize {out['eval_resize']} is smaller than the {out['size']} x {out['size']} centre crop")
    return out


def engine_pixel_norm(args, resolution=None):
    """The EngineOptions.pixel_norm a config's preprocessing keys imply (None when it names none of them).  The datasets normalise 'f32' items on the
    host and the engine normalises every other format on the GPU, so both must use the same statistics: a config whose engine_options carry another
    pixel_norm than its `normalize` (an EngineOptions object always carries one) is a ValueError."""
    pre = preprocess_options(args, resolution)
    eo = args.get("engine_options")
    given = eo.get("pixel_norm") if isinstance(eo, dict) else getattr(eo, "pixel_norm", None)
    want = pre["normalize"] if pre is not None else "imagenet"
    if given is not None and norm_stats(given) != norm_stats(want):
        raise ValueError(f"the datasets normalise with {want!r} (config keys preprocess / normalize) but engine_options.pixel_norm is {given!r}: 'f32' "
                         "items are normalised on the host, every other pixel format by the engine, so the two must agree")
    return None if pre is None else want


def _read(image_root, name):
    with open(os.path.join(image_root, name), "rb") as f:
        return f.read()


class Coco(Dataset):
    """Training pairs of the given tasks (utils/data.py:308-382): item = (image, prompt + pre_caption(caption), 0, task)."""

    def __init__(self, transform=None, image_root=None, ann_file=None, max_words=30, prompt='', tasks=(0,), replay_list=(), pixel_format="f32",
                 size=224, interpolation="bilinear", normalize="imagenet", jpeg_progressive=False, jpeg_layouts=False):
        _pil()
        _check_pixel_format(pixel_format)
        self.jpeg_progressive = _check_jpeg_progressive(jpeg_progressive, pixel_format)
        self.jpeg_layouts = _check_jpeg_layouts(jpeg_layouts, pixel_format)
        _check_filter(interpolation)
        norm_stats(normalize)
        # interpolation / normalize: of the default transforms (an explicit `transform` wins); 'u8', 'decoded' and 'jpeg' items are normalised on the
        # GPU (EngineOptions.pixel_norm), 'f32' items here
        plain = (interpolation, normalize) == ("bilinear", "imagenet") and size == 224
        if transform is None and pixel_format == "u8":
            transform = lambda im: train_transform(im, size, pixel_format="u8", interpolation=interpolation)  # noqa: E731
        if transform is None and pixel_format == "f32" and not plain:
            transform = lambda im: train_transform(im, size, interpolation=interpolation, normalize=normalize)  # noqa: E731
        if transform is None and pixel_format == "decoded":      # size: the S of the output (the default transforms' 224)
            transform = decoded_transform("train", size, interpolation=interpolation)
        self._encoded = transform is None and pixel_format == "jpeg"     # the transform then takes the file's bytes
        if self._encoded:
            transform = encoded_transform("train", size, interpolation=interpolation, progressive=self.jpeg_progressive, layouts=self.jpeg_layouts)
        self.pixel_format, self.interpolation, self.normalize = pixel_format, interpolation, normalize
        with open(ann_file, 'r') as f:
            records = json.load(f)
        cats = {TASK_CATEGORIES[int(t)] for t in tasks}
        self.transform = transform or train_transform
        self.image_root, self.max_words, self.prompt = image_root, max_words, prompt
        self.img_ids = {}
        self.annotation = []
        for ann in records:
            if ann['category'] in cats:
                self.img_ids.setdefault(ann['image_id'], len(self.img_ids))
                self.annotation.append(ann)
        self.annotation += list(replay_list)

    def __len__(self):
        return len(self.annotation)

    def __getitem__(self, index):
        ann = self.annotation[index]
        if self._encoded:
            image = self.transform(_read(self.image_root, ann['image']))
        else:
            image = _load(self.image_root, ann['image'], self.transform)
        return image, self.prompt + pre_caption(ann['caption'], self.max_words), 0, task_of_category(ann['category'])


class CocoEval(Dataset):
    """Evaluation images of tasks 0..t with every caption of every image in the lookup tables the scoring loop reads
    (utils/data.py:186-306; sprompt.py:433-548): text, text_cat, image, txt2img, img2txt; item = (image, image index, task)."""

    def __init__(self, transform=None, image_root=None, ann_file=None, max_words=30, tasks=(0,), eval_transform='center', pixel_format="f32",
                 size=224, resize=256, interpolation="bilinear", normalize="imagenet", jpeg_progressive=False, jpeg_layouts=False):
        _pil()
        _check_pixel_format(pixel_format)
        self.jpeg_progressive = _check_jpeg_progressive(jpeg_progressive, pixel_format)
        self.jpeg_layouts = _check_jpeg_layouts(jpeg_layouts, pixel_format)
        _check_filter(interpolation)
        norm_stats(normalize)
        plain = (interpolation, normalize) == ("bilinear", "imagenet") and (size, resize) == (224, 256)

        def host(pf):      # the host transform of 'u8' / 'f32' with this dataset's geometry, filter and statistics
            if eval_transform == 'center':
                return lambda im: test_transform(im, resize, size, pixel_format=pf, interpolation=interpolation, normalize=normalize)
            return lambda im: train_transform(im, size, pixel_format=pf, interpolation=interpolation, normalize=normalize)
        if transform is None and pixel_format == "u8":
            transform = host("u8")
        if transform is None and pixel_format == "f32" and not plain and eval_transform in ('center', 'reference'):
            transform = host("f32")
        if transform is None and pixel_format == "decoded" and eval_transform in ('center', 'reference'):
            # size / resize: the S and Resize of the output (the default transforms' 224 / 256; CLIP's own preprocessing is resize == size);
            # 'reference' takes the training form
            transform = decoded_transform("center" if eval_transform == 'center' else "train", size, resize, interpolation)
        self._encoded = transform is None and pixel_format == "jpeg" and eval_transform in ('center', 'reference')
        if self._encoded:
            transform = encoded_transform("center" if eval_transform == 'center' else "train", size, resize, interpolation, self.jpeg_progressive,
                                          self.jpeg_layouts)
        self.pixel_format, self.interpolation, self.normalize = pixel_format, interpolation, normalize
        with open(ann_file, 'r') as f:
            records = json.load(f)
        cats = {TASK_CATEGORIES[int(t)] for t in tasks}
        # eval_transform (args['eval_transform'], recorded in the result file): 'center' = the deterministic Resize + CenterCrop the reference
        # defines for evaluation; 'reference' = what the reference's CocoEval actually applies when constructed as sprompt.py:169 does — its default
        # argument is the TRAINING transform (utils/data.py:206: RandomResizedCrop + flip), so R@K of a parity run against the reference code as
        # written needs 'reference'.  An explicit `transform` wins over both.
        if eval_transform not in ('center', 'reference'):
            raise ValueError(f"eval_transform must be 'center' or 'reference', not {eval_transform!r}")
        self.eval_transform = eval_transform
        self.transform = transform or (test_transform if eval_transform == 'center' else train_transform)
        self.image_root, self.max_words = image_root, max_words
        self.ann = [a for a in records if a['category'] in cats]
        self.text, self.text_cat, self.image = [], [], []
        self.txt2img, self.img2txt = {}, {}
        for img_id, ann in enumerate(self.ann):
            self.image.append(ann['image'])
            self.img2txt[img_id] = []
            task = task_of_category(ann['category'])
            for caption in ann['caption']:
                txt_id = len(self.text)
                self.text.append(pre_caption(caption, self.max_words))
                self.text_cat.append(task)
                self.img2txt[img_id].append(txt_id)
                self.txt2img[txt_id] = img_id

    def __len__(self):
        return len(self.ann)

    def __getitem__(self, index):
        ann = self.ann[index]
        if self._encoded:
            return self.transform(_read(self.image_root, ann['image'])), index, task_of_category(ann['category'])
        return _load(self.image_root, ann['image'], self.transform), index, task_of_category(ann['category'])
