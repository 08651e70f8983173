"""Sketch edits with one crop per group of stroke clusters, pasted into one photo.

A sketch edit (chronoedit_amd/sketch.py) puts ONE box around every kept stroke: a mug sketched in one corner of a photo and a hat in the
opposite one give a box that is the whole photo.  With `enable_sketch_region(max_crops=G)`, G >= 2, the clusters of the grown plane
(chronoedit_amd/components.py) are grouped, each group is edited as a focused crop of its own, and the crops are pasted into ONE photo:

    chain     changed -> grown -> roots(grown) -> sums(roots, weight = changed) -> kept (sketch.labelled_stages; min_stroke == 0: kept = grown)
    table     one row per kept cluster - a root r with kept[r] != 0 - in ascending label order: label, left, top, right, bottom (the
              half-open bounding box of its pixels), their number, sums[label], 0.  int32 [ROWS, 8], rows at and after the count 0; the
              count is exact even above ROWS (the rows are then unspecified, and the caller reports "many")
    group     pure integer host code.  Every cluster starts as a group.  A group's extent is the union of its rows' boxes widened by the
              feather on every side and clipped to the photo, its trial box focus.focus_box(extent).  While two trial boxes share a pixel,
              the first such pair (i, j) in group order merges; then, while there are more than max_crops groups, the pair whose union's
              trial box is smallest (ties: the first) merges, and the first rule runs again.  Every step removes a group.  The groups are
              ordered by their smallest label: the paste order
    select    per group 255 where kept != 0 and the pixel's root is one of the group's labels, else 0 - then sketch.box, horizontal and
              vertical, radius feather: the group's mask.  Its final box is focus_box of the EXACT bounding box of that mask, as the
              single-box call's is of the union mask's: final boxes may differ a little from the trial boxes and may overlap - the masks
              decide what is pasted
    paste     per frame canvas = background.copy(); for each group in order canvas.paste(frame_g.resize(box_g size, LANCZOS), box_g[:2],
              mask_g.crop(box_g)) - PIL's paste (((t >> 8) + t) >> 8), chained; composite=False: without the mask (`host_paste`)

What follows from the arithmetic: the selected planes partition `kept`; a pixel within `grow` of a kept changed pixel has its whole feather
window - which reaches grow + feather, the radius of the growth - inside one cluster, so it is 255 in exactly one group's mask and 0 in all
others; and where every group's mask is 0 the output carries the background's bytes.

The functions below are THE definition (numpy and torch on CPU tensors) and the host path; for CUDA tensors `table` and `select` are the
passes of csrc/ce_clusters.hip - integers only, the same bits.  How a checkpoint edits two crops of one photo consistently is the
checkpoint's business."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import components as _cc
from .focus import Box, focus_box

ENTRY_POINTS = ("ce_clusters_table_i32", "ce_clusters_select_u8", "ce_clusters_paste_u8")
ROWS = 256  # rows of the table (CL_ROWS of csrc/ce_clusters.hip)
MAX_CROPS = 16


def check_max_crops(v) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= MAX_CROPS:
        raise ValueError(f"sketch region: max_crops must be an int in 1..{MAX_CROPS}, got {v!r}")
    return v


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def _table_np(roots: np.ndarray, sums: np.ndarray, kept: np.ndarray) -> Tuple[int, np.ndarray]:
    H, W = roots.shape
    r, s, k = roots.reshape(-1), sums.reshape(-1), kept.reshape(-1) != 0
    labels = np.flatnonzero((r == np.arange(r.size, dtype=np.int64)) & k)  # ascending
    out = np.zeros((ROWS, 8), dtype=np.int32)
    lab = labels[:ROWS]
    c = lab.size
    if c:
        at = np.flatnonzero((r >= 0) & k)
        row = np.searchsorted(lab, r[at])
        hit = (row < c) & (lab[np.minimum(row, c - 1)] == r[at])
        at, row = at[hit], row[hit]
        y, x = at // W, at % W
        box = np.stack([np.full(c, W), np.full(c, H), np.zeros(c, np.int64), np.zeros(c, np.int64)])
        np.minimum.at(box[0], row, x), np.minimum.at(box[1], row, y), np.maximum.at(box[2], row, x + 1), np.maximum.at(box[3], row, y + 1)
        out[:c, 0], out[:c, 1:5], out[:c, 5], out[:c, 6] = lab, box.T, np.bincount(row, minlength=c), s[lab]
    return int(labels.size), out


def table(roots: torch.Tensor, sums: torch.Tensor, kept: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (count int32 [1], rows int32 [ROWS, 8]) where the planes lie; on the device nothing is read back."""
    _cc._check_plane(roots, "roots", torch.int32), _cc._check_plane(sums, "sums", torch.int32), _cc._check_plane(kept, "kept")
    if not (roots.shape == sums.shape == kept.shape) or not (roots.device == sums.device == kept.device):
        raise ValueError(f"clusters: roots {tuple(roots.shape)}, sums {tuple(sums.shape)} and kept {tuple(kept.shape)} must share shape and device")
    if roots.is_cuda:
        from . import ops
        rows, counters = ops.clusters_table_i32(roots.contiguous(), sums.contiguous(), kept.contiguous())
        return counters[:1], rows
    count, rows = _table_np(roots.contiguous().numpy(), sums.contiguous().numpy(), kept.contiguous().numpy())
    return torch.tensor([count], dtype=torch.int32), torch.from_numpy(rows)


# ---- the grouping ---------------------------------------------------------------------------------------------------------------------
def extent(rows: Sequence[Sequence[int]], members: Sequence[int], src_size: Tuple[int, int], feather_px: int) -> Box:
    """The union of the members' boxes, widened by feather_px on every side and clipped to the photo."""
    SW, SH = int(src_size[0]), int(src_size[1])
    f = int(feather_px)
    return (max(min(int(rows[i][1]) for i in members) - f, 0), max(min(int(rows[i][2]) for i in members) - f, 0),
            min(max(int(rows[i][3]) for i in members) + f, SW), min(max(int(rows[i][4]) for i in members) + f, SH))


def trial_box(rows, members, src_size, edit_size, context: float, feather_px: int) -> Tuple[Box, str]:
    return focus_box(extent(rows, members, src_size, feather_px), src_size, edit_size, context)


def intersect(a: Box, b: Box) -> bool:
    """Two half-open rectangles share at least one pixel."""
    return a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]


def group(rows, src_size: Tuple[int, int], edit_size: Tuple[int, int], context: float, feather_px: int, max_crops: int) -> List[List[int]]:
    """rows: the table's first `count` rows (a list of lists, an array or a tensor on the host) -> the groups as lists of row indices, in
    paste order.  A pure function of its arguments."""
    check_max_crops(max_crops)
    rows = [[int(v) for v in r] for r in (rows.tolist() if hasattr(rows, "tolist") else rows)]
    groups = [[i] for i in range(len(rows))]
    seen = {}  # members -> trial box: a merge changes one group, and the second rule asks for every pair's union again and again

    def box(members) -> Box:
        key = tuple(sorted(members))
        if key not in seen:
            seen[key] = trial_box(rows, key, src_size, edit_size, context, feather_px)[0]
        return seen[key]

    def merge(i: int, j: int):
        groups[i] = sorted(groups[i] + groups[j])
        del groups[j]

    def first_rule():
        while True:  # ends: every trip but the last removes a group
            boxes = [box(g) for g in groups]
            pair = next(((i, j) for i in range(len(groups)) for j in range(i + 1, len(groups)) if intersect(boxes[i], boxes[j])), None)
            if pair is None:
                return
            merge(*pair)

    first_rule()
    while len(groups) > max_crops:  # ends: every trip removes at least one group
        area = lambda b: (b[2] - b[0]) * (b[3] - b[1])
        _, i, j = min((area(box(groups[i] + groups[j])), i, j) for i in range(len(groups)) for j in range(i + 1, len(groups)))
        merge(i, j)
        first_rule()
    return sorted(groups, key=lambda g: rows[g[0]][0])  # (rows are in ascending label order: g[0] holds the smallest label)


# ---- the masks ------------------------------------------------------------------------------------------------------------------------
def select(roots: torch.Tensor, kept: torch.Tensor, labels_of_group) -> torch.Tensor:
    """THE definition: uint8 [H, W], 255 where kept != 0 and the pixel's root is one of labels_of_group, else 0 (host tensors)."""
    labels = torch.as_tensor(sorted(int(v) for v in labels_of_group), dtype=torch.int32)
    return ((kept != 0) & torch.isin(roots, labels)).to(torch.uint8) * 255


def group_of_row(groups: List[List[int]]) -> torch.Tensor:
    """int32 [ROWS]: the group of every row, -1 for a row in no group - what the device's select pass takes."""
    out = torch.full((ROWS,), -1, dtype=torch.int32)
    for g, members in enumerate(groups):
        out[torch.as_tensor(members, dtype=torch.long)] = g
    return out


def group_masks(roots: torch.Tensor, kept: torch.Tensor, rows_where: torch.Tensor, rows, groups: List[List[int]], feather_px: int) -> List[torch.Tensor]:
    """Per group its mask uint8 [H, W] where the planes lie: the selected plane through sketch.box, horizontal then vertical.  On the device
    one small upload (the rows' groups), then three launches per group; nothing is read back."""
    from . import sketch as _sk
    out = []
    if roots.is_cuda:
        from . import ops
        gor = group_of_row(groups).to(roots.device)
    for g, members in enumerate(groups):
        if roots.is_cuda:
            m = ops.clusters_select_u8(roots, kept, rows_where, gor, g)
        else:
            m = select(roots, kept, [rows[i][0] for i in members])
        if feather_px:
            m = _sk.box(_sk.box(m, feather_px, 0), feather_px, 1)
        out.append(m)
    return out


# ---- one editor value -----------------------------------------------------------------------------------------------------------------
@dataclass
class Crops:
    """What `plan` decided for one editor value."""
    reason: str  # "single" / "crops" / "many" / "unfit"
    groups: List[List[int]] = field(default_factory=list)  # row indices per group (empty for "many")
    labels: List[List[int]] = field(default_factory=list)  # the clusters' labels per group
    plans: list = field(default_factory=list)  # "crops": one focus.FocusPlan per group, in paste order


def plan(e: dict, max_crops: int, width: int, height: int, context: float) -> Crops:
    """One `sketch.masks` entry (made with max_crops >= 2: it holds "count", "rows" and the planes "roots", "kept", "table") -> its Crops.
    G >= 2 groups cost ONE more host read on the device path: the groups' bbox_counts, five integers each, concatenated.
    The reasons in the order they are tested: "many" (more clusters than the table holds), "unfit" (some group's trial box is not "ok" -
    also when the merges left one group, whose box is then the whole photo), "single" (one group with an "ok" box), then "unfit" again
    for a final box that is not "ok", else "crops"."""
    from . import autofocus as _af
    from .focus import FocusPlan
    count, rows = e["count"], e["rows"]
    if count > ROWS:
        return Crops("many")
    SW, SH = e["background"].size
    src, edit = (SW, SH), (int(width), int(height))
    groups = group(rows[:count], src, edit, context, e["feather_px"], max_crops)
    labels = [[rows[i][0] for i in g] for g in groups]
    if any(trial_box(rows, g, src, edit, context, e["feather_px"])[1] != "ok" for g in groups):
        return Crops("unfit", groups, labels)
    if len(groups) < 2:
        return Crops("single", groups, labels)
    masks = group_masks(e["roots"], e["kept"], e["table"], rows, groups, e["feather_px"])
    counts = torch.cat([_af.bbox_counts(m) for m in masks]).tolist()  # (the second read: 5 G integers)
    plans = []
    for g, m in enumerate(masks):
        l, t, r, b, n = (int(v) for v in counts[5 * g:5 * g + 5])
        box, reason = focus_box((l, t, r, b) if n else None, src, edit, context)
        if reason != "ok":
            return Crops("unfit", groups, labels)
        report = {"box": box, "reason": reason, "source_size": src, "edit_size": edit, "scale": (box[2] - box[0]) / edit[0],
                  "mask_fraction_of_box": float(n) / ((box[2] - box[0]) * (box[3] - box[1]))}
        if "mask_dev" in e:
            plans.append(FocusPlan.make(e["composite"], report, m, m.device, e["background"], uploaded=(e["cp_u8"], e["bg_u8"])))
        else:
            plans.append(FocusPlan.make(e["composite"], report, m, paste_image=e["background"]))
    return Crops("crops", groups, labels, plans)


def crop_reports(crops: Crops, single) -> list:
    """The report's "crops" list - what ran, in paste order: the groups' plans, or the single-box plan (`single`, a focus.FocusPlan) with
    every kept cluster's label (None where no grouping was made: "many", no strokes, or max_crops == 1).  The masks are copied to the host here."""
    from PIL import Image
    if crops.reason == "crops":
        pairs = list(zip(crops.plans, crops.labels))
    else:
        pairs = [(single, sorted(v for g in crops.labels for v in g) if crops.labels else None)]
    keys = ("box", "reason", "scale", "mask_fraction_of_box")
    return [dict({k: p.report[k] for k in keys}, clusters=labels, mask=Image.fromarray(p.host_mask().numpy(), mode="L")) for p, labels in pairs]


# ---- the output -----------------------------------------------------------------------------------------------------------------------
def host_paste(background, frames_of_group: list, masks: Optional[list], boxes: List[Box]) -> list:
    """THE definition of the output.  frames_of_group[g]: group g's frames (PIL, the edit's size); masks[g]: its photo-size mask uint8 [SH,
    SW] on the host (masks None: composite=False, whole boxes are replaced); boxes[g] its final box -> per frame a PIL image of the
    photo's size."""
    from PIL import Image
    src = background.convert("RGB")
    out = []
    for f in range(len(frames_of_group[0])):
        canvas = src.copy()
        for g, (l, t, r, b) in enumerate(boxes):
            m = None if masks is None else Image.fromarray(masks[g].numpy()).crop((l, t, r, b))
            canvas.paste(frames_of_group[g][f].resize((r - l, b - t), Image.LANCZOS), (l, t), m)
        out.append(canvas)
    return out


def paste(video: torch.Tensor, plans: list, crop_of: List[Tuple[int, int]], output_type: str, composite: bool, lift=None, report: Optional[list] = None,
          mask_aware: bool = False):
    """focus.paste for a flat list of crops: sample b is crop crop_of[b] = (value, g) of its editor value, g counting from 0 in paste order;
    the crops of one value are chained into ONE video at the photo's size (`host_paste`; on the device ce_focus_paste_u8 builds the canvas
    from the background with the first crop, ce_clusters_paste_u8 adds the others in place) -> one entry per value, in postprocess_video's
    layouts.  lift: a lift.LiftConfig - every crop is lifted inside its box from its plan's `lift_L` before the paste (boxlift.output), in
    the same order, and `report` receives one `lift_report` entry per crop; mask_aware: the fits run under the plans' `lift_M`."""
    from . import focus as _fc
    from . import image_io, ops
    image_io.check_output_type(output_type)
    if lift is not None:
        from . import boxlift
        frames, entries = boxlift.output(video, plans, None, crop_of, lift, output_type, composite, mask_aware)
        if report is not None:
            report.extend(entries)
        return frames
    on_device = plans[0].src_u8 is not None and image_io.device_video(video)
    u8 = ops.video_to_u8(video.contiguous()) if on_device else None
    values = sorted({v for v, _ in crop_of})
    out = []
    for v in values:
        members = [b for b, (vb, _) in enumerate(crop_of) if vb == v]  # (ascending b is ascending g)
        ps = [plans[b] for b in members]
        if on_device:
            first = ps[0]
            canvas = _fc.device_paste(u8[members[0]], first.src_u8 if first.paste_u8 is None else first.paste_u8,
                                      first.mask_dev if composite else None, first.box)
            for b, p in zip(members[1:], ps[1:]):
                l, t, r, b_ = p.box
                frames = u8[b]
                if tuple(frames.shape[1:3]) != (b_ - t, r - l):
                    frames = torch.stack([image_io.resize_u8(f, (r - l, b_ - t), image_io.LANCZOS) for f in frames])
                ops.clusters_paste_u8(frames.contiguous(), p.mask_dev if composite else None, canvas, l, t)
            out.append(canvas.cpu().numpy())
        else:
            frames = [image_io.postprocess_video(video[b:b + 1], "pil")[0] for b in members]
            first = ps[0]
            pasted = host_paste(first.image if first.paste_image is None else first.paste_image, frames,
                                [p.host_mask() for p in ps] if composite else None, [p.box for p in ps])
            out.append(np.stack([np.asarray(f, dtype=np.uint8) for f in pasted]))
    return image_io.frames_from_u8(out, output_type)
