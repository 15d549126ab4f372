"""numpy restatement of the target rule of include/vitadapter_hip_seg_target.h (the reference's ToMask step,
formatting.py:58-77, for a batch): what the seg_targets tests compare with, and the cases they share.  Not a test module.

Rule per image: g = remap[label] where a table is given (every entry on the original value), the labels are np.unique(g)
without ignore_index, mask k is g == labels[k]."""
import numpy as np


def targets(maps, ignore_index=255, remap=None):
    """maps (N, H, W) integers -> dict(masks (G, H, W) uint8, labels (G,) int64, image_of (G,) int32, counts [N], offsets [N + 1])"""
    maps = np.asarray(maps)
    N, H, W = maps.shape
    g = maps.astype(np.int64)
    if remap is not None:
        g = np.asarray(remap).astype(np.int64)[g]
    masks, labels, image_of, counts = [], [], [], []
    for n in range(N):
        lab = np.unique(g[n])
        lab = lab[lab != ignore_index]
        counts.append(int(lab.size))
        for v in lab:
            masks.append((g[n] == v).astype(np.uint8))
            labels.append(int(v))
            image_of.append(n)
    return dict(masks=np.stack(masks) if masks else np.zeros((0, H, W), np.uint8), labels=np.asarray(labels, dtype=np.int64),
                image_of=np.asarray(image_of, dtype=np.int32), counts=counts,
                offsets=[int(sum(counts[:n])) for n in range(N + 1)])


def lists(maps, ignore_index=255, remap=None):
    """-> (gt_labels, gt_masks): per image (G_n,) int64 and (G_n, H, W) int64, what the reference's pipeline hands the head"""
    t = targets(maps, ignore_index, remap)
    o = t['offsets']
    return ([t['labels'][a:b] for a, b in zip(o, o[1:])], [t['masks'][a:b].astype(np.int64) for a, b in zip(o, o[1:])])


def reduce_zero_table():
    """mmseg's reduce_zero_label as a table: 0 and 255 -> 255, else v - 1"""
    return np.array([255 if v in (0, 255) else v - 1 for v in range(256)], dtype=np.uint8)


def case_maps():
    """name -> (N, H, W) uint8 map: the cases of the golden (tools/gen_golden_seg_targets.py stores exactly these)"""
    rng = np.random.RandomState(21)
    out = {}
    out['one_pixel'] = np.array([[[7]]], dtype=np.uint8)
    out['one_pixel_ignored'] = np.array([[[255]]], dtype=np.uint8)
    out['all_values'] = rng.permutation(256).astype(np.uint8).reshape(1, 16, 16)
    # odd widths; image 1 all ignored; class 9 only in image 0; class 4 only in the last pixel of image 2
    m = rng.choice(np.array([0, 1, 3, 255], dtype=np.uint8), size=(3, 7, 13))
    m[0, 2, 5:9] = 9
    m[1] = 255
    m[2, 6, 12] = 4
    out['odd'] = m
    # 12576 pixels an image: several workgroup ranges; class 77 only in the last range of image 1, 200 only at its very end
    m = (rng.randint(0, 6, size=(2, 12, 17)).repeat(8, axis=1).repeat(8, axis=2)[:, :, :131]).astype(np.uint8)
    m[0, 40:50, 60:90] = 255
    m[1, 95, 100:120] = 77
    m[1, 95, 130] = 200
    out['ranges'] = m
    out['mapillary'] = np.concatenate([np.arange(66), rng.randint(0, 66, size=6 * 12 - 66)]).astype(np.uint8).reshape(1, 6, 12)
    out['reduce_zero'] = rng.choice(np.array([0, 1, 2, 150, 254, 255], dtype=np.uint8), size=(2, 5, 9))
    return out


# name -> (map name, ignore_index, remap name or None); remap 'mapillary' is the golden's stored table
CASES = {
    'one_pixel': ('one_pixel', 255, None),
    'one_pixel_ignored': ('one_pixel_ignored', 255, None),
    'all_values_255': ('all_values', 255, None),
    'all_values_0': ('all_values', 0, None),
    'all_values_neg': ('all_values', -100, None),
    'odd': ('odd', 255, None),
    'ranges': ('ranges', 255, None),
    'mapillary': ('mapillary', 255, 'mapillary'),
    'reduce_zero': ('reduce_zero', 255, 'reduce_zero'),
}
OUT_OF_RANGE = np.array([[[3, 300, 3, -1], [255, 3, 0, 300]], [[0, 0, 0, 0], [255, 255, 255, 255]]], dtype=np.int64)
