"""Device-resident RGB-T tracking loop: the host side of the reference trackers
(lib/test/tracker/mixformer_vit_rgbt.py, mixformer_vit_rgbt_shared.py, asymmetric_shared.py,
asymmetric_shared_online.py) with their per-frame work moved onto the MI355X.

Per frame the reference does, on the host: two cv2 crops (sample_target), the preprocessor
(H2D copy, /255, normalise; cv2.applyColorMap JET on the TIR crop for the multimodal
preprocessor), the network forward, `.tolist()` of the box (a device sync), map_box_back and
clip_box in Python (tracker.py:75-106).  Here one tracking step is ONE hipGraph replay of
  mmt_sample_target (both search crops, computed from the device-resident state)
  -> the model's launch plan (zero-copy: its patch staging reads the crop buffers in place)
  -> mmt_track_update (box scaling, map_box_back, clip_box; the state is updated on the device)
and the only host round trip is the one the API needs: returning `target_bbox` as a list (and,
for the online-score tracker, its `pred_score.item()` decision, as in the reference).

The arithmetic of both kernels follows the reference bit for bit where it is pinned (crop
geometry and padding, map-back, clip) and OpenCV's fixed-point resize / colour map where cv2
would run (see csrc/preprocess.hip; oracle/preprocess.py restates both).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import DEPTH_WORK_BYTES, LIB, CropParams, DepthParams, check
from .depth import as_depth16, check_aux_format, depth_params

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def jet_lut():
    """[256][3] (B, G, R) uint8 JET colour map: the piecewise-linear jet of OpenCV's COLORMAP_JET,
    x = i / 255 (r = clip(min(4x - 1.5, 4.5 - 4x)), g = .. 0.5 / 3.5, b = .. -0.5 / 2.5), x255, rounded."""
    x = np.arange(256, dtype=np.float64) / 255.0
    r = np.clip(np.minimum(4 * x - 1.5, -4 * x + 4.5), 0, 1)
    g = np.clip(np.minimum(4 * x - 0.5, -4 * x + 3.5), 0, 1)
    b = np.clip(np.minimum(4 * x + 0.5, -4 * x + 2.5), 0, 1)
    lut = np.stack([b, g, r], 1).astype(np.float32) * np.float32(255.0)
    return np.clip(np.rint(lut), 0, 255).astype(np.uint8)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def crop_params(image, box, factor, out_sz, out=None, patch=None, crop=None, lut=None):
    """mmt_crop_params for one crop.  image (H,W,3) uint8, box (4,) fp64, out (1,3,s,s) fp32,
    patch (s,s,3) uint8, crop (4,) fp64, lut (256,3) uint8 -- all device tensors."""
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or not image.is_contiguous():
        raise ValueError("image must be a contiguous (H, W, 3) uint8 device tensor")
    if box.dtype != torch.float64 or box.numel() != 4:
        raise ValueError("box must be 4 float64 values (x, y, w, h)")
    for t, shape, dt in ((out, (3 * out_sz * out_sz,), torch.float32), (patch, (out_sz * out_sz * 3,), torch.uint8),
                         (crop, (4,), torch.float64), (lut, (768,), torch.uint8)):
        if t is not None and (t.dtype != dt or t.numel() != shape[0] or not t.is_contiguous() or t.device != image.device):
            raise ValueError("crop buffer of shape %s / %s on %s expected" % (shape, dt, image.device))
    p = CropParams()
    p.image, p.H, p.W = image.data_ptr(), image.shape[0], image.shape[1]
    p.box, p.factor, p.out_sz = box.data_ptr(), float(factor), int(out_sz)
    p.lut = _ptr(lut)
    for c in range(3):
        p.mean[c], p.std[c] = MEAN[c], STD[c]
    p.out, p.patch, p.crop = _ptr(out), _ptr(patch), _ptr(crop)
    return p


def sample_target(params_list, stream=None):
    """Launch mmt_sample_target for up to 4 crops of equal out_sz."""
    n = len(params_list)
    arr = (CropParams * n)(*params_list)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(LIB.mmt_sample_target(arr, n, s), "mmt_sample_target")
    return arr


def check_depth_frame(x, H, W):
    """aux_format="depth16": the second frame of a pair as an int16 tensor holding the uint16 bits (as_depth16),
    of the RGB frame's size; ValueError otherwise."""
    d = as_depth16(x, "the depth frame")
    if tuple(d.shape) != (H, W):
        raise ValueError("the depth frame must be (%d, %d), the RGB frame's size, got %s" % (H, W, tuple(d.shape)))
    return d


def _split_pair(image):
    """aux_format="depth16": [image_v, image_i] checked as a (H, W, 3) uint8 frame and a (H, W) 16-bit depth
    frame.  Returns (H, W, rgb, depth) as torch tensors (host or device)."""
    if not isinstance(image, (list, tuple)) or len(image) != 2:
        raise ValueError("image must be [image_v, image_i]")
    ims = [torch.as_tensor(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) and x.dtype != np.uint16 else x
           for x in image]
    rgb = ims[0]
    if not isinstance(rgb, torch.Tensor) or rgb.dim() != 3 or rgb.shape[2] != 3 or rgb.dtype != torch.uint8:
        raise ValueError("the RGB frame must be a (H, W, 3) uint8 image")
    H, W = rgb.shape[:2]
    if H <= 0 or W <= 0:
        raise ValueError("the RGB frame must be a (H, W, 3) uint8 image")
    return H, W, rgb, check_depth_frame(ims[1], H, W)


class RGBTTrackerCore:
    """Tracking state and per-frame step of one sequence on the current device.

    network: a built HIP model (mmt_amd.model); multimodal: apply the JET colour map to the TIR
    crops (Preprocessor_Multimodal) or not (Preprocessor_wo_mask); online_score: the
    asymmetric_shared_online tracker's score-gated online-template update; online_size / max_score_decay:
    upstream's memory of K online templates and its score decay (online_memory_schedule; online-score tracker
    only, the network set to the same size with set_online_size).

    aux_format: "rgb8" (default): image[1] is a (H, W, 3) uint8 frame.  "depth16" (RGB-D): image[1] is the raw
    (H, W) depth frame of the RGB frame's size -- numpy uint16, torch uint16, or torch int16 taken as the bit
    pattern of the uint16 values, on the host or already on the device.  It is copied into a uint16 device buffer
    and prepared on the device (mmt_amd.depth: clip at 3 x median, min-max normalise, three channels) into the
    second-modality frame buffer: eagerly before the template crop in `initialize`, as the first launches of
    the step graph in `track`.  Everything after reads that buffer as it reads an uploaded frame.  The step is
    then built from the table forms (mmt_depth_prepare_table, mmt_sample_target_table, mmt_track_update_slots,
    one slot): same arithmetic, and a new frame size rewrites the table entries and keeps the graph."""

    def __init__(self, network, template_factor, template_size, search_factor, search_size, update_intervals,
                 multimodal, online_score=False, use_graph=True, kv_cache=False, online_size=1, max_score_decay=1.0,
                 aux_format="rgb8"):
        self.aux_format = check_aux_format(aux_format)
        self.net = network
        # online_size K > 1 (online-score tracker): K online templates, filled and replaced by upstream's
        # score-gated ring (online_memory_schedule).  The step always runs the cached passes, as upstream runs
        # set_online / forward_test; a promotion writes one template slot and the sequence's length, and replays
        # the captured template pass: nothing is re-planned or re-captured.  K = 1 with decay 1.0: the code below
        # as it was.
        self.online_size, self.max_score_decay = check_online_memory(online_size, max_score_decay, online_score, network)
        self._ring = self.online_size > 1 or self.max_score_decay != 1.0
        self.online_count, self.forget_id = 1, 0
        kv_cache = kv_cache or self.online_size > 1
        # kv_cache: the template tokens' per-layer qkv are computed once per template update (a
        # separate template pass) and each frame runs only the search tokens (runtime.cache_workspace);
        # off by default: no faster at batch 1 (lib/test/tracker/_rgbt.py KV_CACHE_DEFAULT)
        self.kv_cache = bool(kv_cache)
        self._tmpl_dirty = True
        self._tmpl_graph = self._tmpl_plan = None
        self.tf, self.ts, self.sf, self.ss = float(template_factor), int(template_size), float(search_factor), int(search_size)
        self.update_intervals = list(update_intervals)
        self.online_score = bool(online_score)
        self.use_graph = bool(use_graph)
        self.dev = torch.device("cuda", torch.cuda.current_device())
        dev = self.dev
        self.lut = torch.from_numpy(jet_lut().reshape(-1)).to(dev) if multimodal else None
        e = lambda *s, dt=torch.float32: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
        self.state = e(4, dt=torch.float64)
        self.template = [e(1, 3, self.ts, self.ts) for _ in range(2)]
        self.online_template = [e(1, 3, self.ts, self.ts) for _ in range(2)]
        if self.online_size > 1:
            self.online_template = [torch.zeros(1, self.online_size, 3, self.ts, self.ts, device=dev) for _ in range(2)]
        self.online_max_template = [e(1, 3, self.ts, self.ts) for _ in range(2)]
        self.search = [e(1, 3, self.ss, self.ss) for _ in range(2)]
        self.search_crop = e(2, 4, dt=torch.float64)
        self.tmpl_crop = e(2, 4, dt=torch.float64)
        self.frames = None
        self._graph = None
        self._plan = None
        self._rt = None
        self._tmpl_graph = None
        self.frame_id = 0
        self.max_pred_score = -1.0
        if self.aux_format == "depth16":  # device tables of one slot: two crop entries, one depth entry
            self._dbuf = self._fbuf = self._hw = self._depth = self._depth_host = None
            self._dwork = torch.empty(DEPTH_WORK_BYTES, device=dev, dtype=torch.uint8)
            self._search_tab = torch.zeros(2 * ctypes.sizeof(CropParams), device=dev, dtype=torch.uint8)
            self._depth_tab = torch.zeros(ctypes.sizeof(DepthParams), device=dev, dtype=torch.uint8)
            self.hw = torch.zeros(1, 2, device=dev, dtype=torch.int32)

    # ------------------------------------------------------------------ frames
    def _load_frames(self, image):
        """Copy the two (H, W, 3) uint8 frames (numpy or torch) into fixed device buffers."""
        if self.aux_format == "depth16":
            return self._load_depth_pair(image)
        if not isinstance(image, (list, tuple)) or len(image) != 2:
            raise ValueError("image must be [image_v, image_i]")
        ims = [torch.as_tensor(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x for x in image]
        H, W = ims[0].shape[:2]
        if any(tuple(x.shape) != (H, W, 3) or x.dtype != torch.uint8 for x in ims):
            raise ValueError("frames must be two (H, W, 3) uint8 images of the same size")
        if self.frames is None or tuple(self.frames[0].shape) != (H, W, 3):
            self.frames = [torch.empty(H, W, 3, device=self.dev, dtype=torch.uint8) for _ in range(2)]
            self._graph = self._plan = None
        for dst, src in zip(self.frames, ims):
            dst.copy_(src, non_blocking=src.device.type == "cuda")
        return H, W

    def _load_depth_pair(self, image):
        """aux_format="depth16": copy the RGB frame and the raw depth frame into device buffers that only grow;
        a new frame size rewrites the table entries the step graph reads (the graph itself stays)."""
        H, W, rgb, depth = _split_pair(image)
        dev, n = self.dev, H * W
        if self._dbuf is None or self._dbuf.numel() < n:
            self._fbuf = [torch.empty(n * 3, device=dev, dtype=torch.uint8) for _ in range(2)]
            self._dbuf = torch.empty(n, device=dev, dtype=torch.int16)
            self._hw = None
        if self._hw != (H, W):
            self._hw = (H, W)
            self.frames = [buf[:n * 3].view(H, W, 3) for buf in self._fbuf]
            self._depth = self._dbuf[:n].view(H, W)
            self._depth_host = depth_params(self._depth, self.frames[1], self._dwork)
            crops = (CropParams * 2)(*[crop_params(self.frames[m], self.state, self.sf, self.ss,
                                                   out=self.search[m].view(-1), crop=self.search_crop[m],
                                                   lut=self.lut if m == 1 else None) for m in range(2)])
            self._search_tab.copy_(torch.frombuffer(crops, dtype=torch.uint8))
            self._depth_tab.copy_(torch.frombuffer(self._depth_host, dtype=torch.uint8))
            self.hw.copy_(torch.tensor([[H, W]], dtype=torch.int32))
        self.frames[0].copy_(rgb, non_blocking=rgb.device.type == "cuda")
        self._depth.copy_(depth, non_blocking=depth.device.type == "cuda")
        return H, W

    def _prepare_depth(self):
        """The device preparation of the loaded depth frame into frames[1], eagerly (`initialize`)."""
        check(LIB.mmt_depth_prepare(ctypes.byref(self._depth_host), 1, torch.cuda.current_stream().cuda_stream),
              "mmt_depth_prepare")

    def _crop_templates(self, dst, box):
        """Both modalities' template crops at `box` (device fp64) into dst[0] / dst[1]."""
        ps = [crop_params(self.frames[m], box, self.tf, self.ts, out=dst[m].view(-1), crop=self.tmpl_crop[m],
                          lut=self.lut if m == 1 else None) for m in range(2)]
        sample_target(ps)

    # ------------------------------------------------------------------ per-frame plan
    def _build_step(self):
        rt = self.net._runtime(self.dev)
        # the captured graphs hold raw pointers into this runtime's weights and workspace: keep it
        # alive, and rebuild when the network swaps it (load_state_dict / .to() / refresh_kernels)
        self._rt = rt
        score = self.online_score
        part = "s" if self.kv_cache else None
        model_plan = rt.plan_for_inputs(self.template, self.online_template, self.search, run_score_head=score,
                                        part=part)
        ws = rt.workspace(1)
        if self.kv_cache:
            self._tmpl_plan = rt.plan_for_inputs(self.template, self.online_template, None, part="t")
            self._tmpl_graph = rt.capture_plan(self._tmpl_plan) if self.use_graph else None
            self._tmpl_dirty = True
        self._ws = ws
        if self.aux_format == "depth16":  # the table forms over one slot: the frame size lives in device memory
            plan = [(LIB.mmt_depth_prepare_table, (self._depth_tab.data_ptr(), None, 1), "track_depth_prepare_table", None),
                    (LIB.mmt_sample_target_table, (self._search_tab.data_ptr(), None, 2, self.ss),
                     "track_sample_target_table", None)]
            plan += model_plan
            plan.append((LIB.mmt_track_update_slots, (ws["BOX"].data_ptr(), self.search_crop.data_ptr(), 8,
                                                      self.state.data_ptr(), self.hw.data_ptr(), None, 1, self.ss, 10.0),
                         "track_update_slots", None))
        else:
            H, W = self.frames[0].shape[:2]
            self._keep = [crop_params(self.frames[m], self.state, self.sf, self.ss, out=self.search[m].view(-1),
                                      crop=self.search_crop[m], lut=self.lut if m == 1 else None) for m in range(2)]
            arr = (CropParams * 2)(*self._keep)
            plan = [(LIB.mmt_sample_target, (arr, 2), "track_sample_target", arr)]
            plan += model_plan
            plan.append((LIB.mmt_track_update, (ws["BOX"].data_ptr(), self.search_crop.data_ptr(), self.state.data_ptr(), 1,
                                                H, W, self.ss, 10.0), "track_update", None))
        self._plan = plan
        if self.use_graph:
            # capture_plan runs the plan once before recording it, and mmt_track_update moves the
            # state: keep the state of this frame across the capture
            saved = self.state.clone()
            self._graph = rt.capture_plan(plan)
            self.state.copy_(saved)
        else:
            self._graph = None

    def _step(self):
        if self._plan is not None and self.net._runtime(self.dev) is not self._rt:
            self._graph = self._plan = self._tmpl_graph = None  # weights reloaded: re-plan, re-capture
            self._tmpl_dirty = True
        if self._plan is None or (self.use_graph and self._graph is None):
            self._build_step()
        if self.kv_cache and self._tmpl_dirty:  # template pass after a template / online-template change
            if self.online_size > 1:  # the filled slots: read from device memory by the captured passes
                self._rt.load_online_count(self._ws, [self.online_count])
            if self._tmpl_graph is not None:
                self._tmpl_graph.replay()
            else:
                self._rt.run_plan(self._tmpl_plan)
            self._tmpl_dirty = False
        if self._graph is not None:
            self._graph.replay()
        else:
            self._rt.run_plan(self._plan)

    # ------------------------------------------------------------------ tracker API
    def initialize(self, image, init_bbox):
        self._load_frames(image)
        if self.aux_format == "depth16":
            self._prepare_depth()
        self.state.copy_(torch.tensor([float(v) for v in init_bbox], dtype=torch.float64))
        self._crop_templates(self.template, self.state)
        for m in range(2):
            if self.online_size > 1:  # slot 0 = the template (upstream :68); the other slots are not read yet
                self.online_template[m].zero_()
                self.online_template[m][:, 0].copy_(self.template[m])
            else:
                self.online_template[m].copy_(self.template[m])
            # reference defect D6 (asymmetric_shared_online.py:115): online_max_template is read
            # before it is ever assigned if no frame scores > 0.5 before the first update frame;
            # here it starts as the template instead of raising AttributeError
            self.online_max_template[m].copy_(self.template[m])
        self.frame_id = 0
        self.max_pred_score = -1.0
        self.online_count, self.forget_id = 1, 0
        self._tmpl_dirty = True
        self._check_crop(self.tmpl_crop)

    def track(self, image):
        """One frame: returns the new state [x, y, w, h] (Python floats)."""
        self._load_frames(image)
        self.frame_id += 1
        self._step()
        if self._ring:
            pred_score = torch.sigmoid(self._ws["SC"].view(1)).item()
            crop, writes, (self.online_count, self.forget_id, self.max_pred_score) = online_memory_schedule(
                self.frame_id, self.update_intervals, pred_score, (self.online_count, self.forget_id, self.max_pred_score),
                self.online_size, self.max_score_decay)
            if crop:
                self._crop_templates(self.online_max_template, self.state)
            for j, slot in enumerate(writes):  # the first from the candidate, any further one from the template
                src = self.online_max_template if j == 0 else self.template
                for m in range(2):
                    (self.online_template[m][:, slot] if self.online_size > 1 else self.online_template[m]).copy_(src[m])
            if writes:
                for m in range(2):
                    self.online_max_template[m].copy_(self.template[m])
                self._tmpl_dirty = True
        elif self.online_score:
            pred_score = torch.sigmoid(self._ws["SC"].view(1)).item()
            if pred_score > 0.5 and pred_score > self.max_pred_score:
                self._crop_templates(self.online_max_template, self.state)
                self.max_pred_score = pred_score
            for update_i in self.update_intervals:
                if self.frame_id % update_i == 0:
                    for m in range(2):
                        self.online_template[m].copy_(self.online_max_template[m])
                        self.online_max_template[m].copy_(self.template[m])
                    self.max_pred_score = -1
                    self._tmpl_dirty = True
        else:
            for update_i in self.update_intervals:
                if self.frame_id % update_i == 0:
                    self._crop_templates(self.online_template, self.state)
                    self._tmpl_dirty = True
        vals = torch.cat([self.state, self.search_crop[:, 2]]).tolist()  # the step's one host round trip
        if min(vals[4:]) < 1:
            raise Exception("Too small bounding box.")  # processing_utils.py:36-37
        self.last_crop_sz = vals[4]  # this frame's RGB search crop side (resize factor = search_size / it)
        return vals[:4]

    def last_pred_box(self):
        """This frame's network box (cx, cy, w, h), normalised to the search crop (one extra host copy)."""
        return self._ws["BOX"].view(-1, 4)[0].tolist()

    def _check_crop(self, crop):
        if float(crop[:, 2].min()) < 1:
            raise Exception("Too small bounding box.")  # processing_utils.py:36-37


# ---------------------------------------------------------------------- N sequences per replay
def template_schedule(online_score, frame_id, update_intervals, pred_score=None, max_pred_score=-1.0):
    """The per-frame template decisions of RGBTTrackerCore.track as a pure function of one slot's
    counters: returns (crop, promotions, max_pred_score).

    Plain trackers: crop = re-crop the online template at the new state (frame_id on an interval).
    Online-score tracker: crop = the score gate (pred_score > 0.5 and > max_pred_score: the crop at
    the new state becomes the candidate, online_max_template); promotions = how many intervals divide
    frame_id: the first promotes the candidate to online template and resets the candidate to the
    template, any further one (the reference's loop runs once per interval) then promotes that reset
    candidate, i.e. the template itself.  max_pred_score is the value after the frame."""
    due = 0
    for i in update_intervals:
        if frame_id % i == 0:
            due += 1
    if not online_score:
        return due > 0, 0, max_pred_score
    crop = pred_score > 0.5 and pred_score > max_pred_score
    if crop:
        max_pred_score = pred_score
    if due:
        max_pred_score = -1
    return crop, due, max_pred_score


def online_memory_schedule(frame_id, update_intervals, pred_score, memory, online_size, max_score_decay=1.0):
    """The online-score tracker's frame with a memory of online_size online templates (upstream
    lib/test/tracker/mixformer_vit_online.py:107-129), as a pure function of one sequence's counters.
    memory = (count, forget_id, max_pred_score): the filled slots (1 after initialize, the template's copy in
    slot 0, :68), the ring's next victim, and the best score since the last update.  Per frame: the best score
    decays; the score gate (pred_score > 0.5 and > max_pred_score) makes the crop at the new state the candidate;
    then every interval that divides frame_id, in order, appends the candidate while count < online_size, else
    overwrites slot forget_id and advances the ring, and resets the candidate to the template and the best
    score to -1 (so a second interval on the same frame stores the template itself).
    Returns (crop, writes, memory'): writes = the slots written, the first from the candidate, any further one
    from the template.  online_size 1 with decay 1.0 makes template_schedule's decisions (writes = [0] * due)."""
    count, forget_id, max_pred_score = memory
    max_pred_score = max_pred_score * max_score_decay
    crop = pred_score > 0.5 and pred_score > max_pred_score
    if crop:
        max_pred_score = pred_score
    writes = []
    for i in update_intervals:
        if frame_id % i == 0:
            if count < online_size:
                writes.append(count)
                count += 1
            else:
                writes.append(forget_id)
                forget_id = (forget_id + 1) % online_size
            max_pred_score = -1
    return crop, writes, (count, forget_id, max_pred_score)


def check_online_memory(online_size, max_score_decay, online_score, network=None):
    """The trackers' online_size / max_score_decay arguments: (K, decay) or ValueError."""
    K, decay = int(online_size), float(max_score_decay)
    if K != online_size or K < 1:
        raise ValueError("online_size must be an integer >= 1, got %r" % (online_size,))
    if not 0.0 < decay <= 1.0:
        raise ValueError("max_score_decay must lie in (0, 1], got %r" % (max_score_decay,))
    if not online_score and (K > 1 or decay != 1.0):
        raise ValueError("online_size > 1 and max_score_decay belong to the online-score tracker: the plain trackers "
                         "re-crop their one online template and have no upstream ring")
    if network is not None and getattr(network, "online_size", 1) != K:
        raise ValueError("the network was built for online_size %d, the tracker asks for %d (network.set_online_size)"
                         % (getattr(network, "online_size", 1), K))
    return K, decay


def pack_rungs(pack, slots):
    """The batch sizes of the packed step, ascending: `pack` None or () -> () (off); "auto" -> slots // 2,
    slots // 4, ..., 1; else a sequence of distinct sizes R with 1 <= R < slots.  ValueError otherwise."""
    slots = int(slots)
    if pack is None:
        return ()
    if isinstance(pack, str):
        if pack != "auto":
            raise ValueError("pack must be None, \"auto\" or a tuple of batch sizes, got %r" % (pack,))
        rungs, r = [], slots // 2
        while r >= 1:
            rungs.append(r)
            r //= 2
        return tuple(sorted(rungs))
    try:
        rungs = [r for r in pack]
    except TypeError:
        raise ValueError("pack must be None, \"auto\" or a tuple of batch sizes, got %r" % (pack,)) from None
    for r in rungs:
        if isinstance(r, bool) or not isinstance(r, int) or not 1 <= r < slots:
            raise ValueError("a packed batch size must be an int in 1..slots-1 (slots=%d), got %r" % (slots, r))
    if len(set(rungs)) != len(rungs):
        raise ValueError("duplicate packed batch size in %r" % (pack,))
    return tuple(sorted(rungs))


def choose_rung(rungs, n_active):
    """The batch a step of n_active slots runs at: the smallest rung >= n_active, or None (the full step)."""
    fit = [r for r in rungs if r >= n_active]
    return min(fit) if fit else None


def pack_list(active, rung):
    """The rung's slot list: the active slots in ascending order, padded with -1 to `rung` entries."""
    act = sorted(int(b) for b in active)
    if len(act) > rung:
        raise ValueError("%d active slots do not fit batch %d" % (len(act), rung))
    return act + [-1] * (rung - len(act))


class RGBTBatchTrackerCore:
    """`slots` sequences tracked together: one tracking step of every slot is ONE hipGraph replay of
      mmt_sample_target_table (2 * slots search crops, read from a crop-descriptor table in device memory)
      -> the model's launch plan at batch `slots` -> mmt_track_update_slots (per-slot frame size, active mask)
    and one host round trip for all slots.  A slot has its own frame size, state, frame counter and
    template schedule (the decisions of RGBTTrackerCore.track, see template_schedule); when its
    sequence ends, `assign` starts the next one in it.  The captured graph holds the table pointer,
    not the frame pointers: a new frame size rewrites the slot's table entries and keeps the graph.

    Arguments as RGBTTrackerCore, plus slots, slot_cache, refresh_slots and pack.  kv_cache (the whole-batch
    template pass) is refused (NotImplementedError): slots update their templates on different frames;
    slot_cache is its per-slot form.

    slot_cache=True: the template K/V cache per slot (runtime.slot_cache_workspace).  The step graph is
    mmt_sample_target_table -> the search-only pass at batch `slots` -> mmt_track_update_slots, and a
    slot whose templates changed is DIRTY: `assign` wrote them, the schedule re-cropped its online
    template (plain trackers) or promoted its candidate (online-score tracker; a candidate crop alone
    does not dirty it).  The dirty slots are refreshed at the start of the next `track`, before the step
    graph, in ascending slot order: ceil(dirty / refresh_slots) replays of one refresh graph (template
    crops gathered by a device slot list, the template pass at batch refresh_slots, K / V rows
    scattered), none when no slot is dirty.  `release` clears the slot's mark; a weight reload marks
    every active slot.  refresh_slots defaults to min(8, slots).  refresh_replays counts the replays.
    Candidate-elimination networks raise the runtime's NotImplementedError at construction.

    pack=(R, ...) or "auto" (pack_rungs; default None: off, the step above and nothing else): when the
    active slots fit a smaller batch, the step runs at the smallest rung R >= len(active) on the active
    slots only: mmt_sample_target_packed (search crops of the slots of a device slot list, into the rung's
    batch-R rows) -> one mmt_slot_copy gathering the listed slots' templates (slot_cache: their K / V rows
    of the N-slot cache) -> the model's plan at batch R in a workspace of the rung's own ->
    mmt_track_update_packed (row j updates slot list[j]).  Each rung has its own plan and graph, built at
    its first use; the list (active slots ascending, padded with -1) is rewritten only when the membership
    changes; the gather runs every step, so a rung holds no state and the refreshes, dirty marks and the
    template schedule are what they are without packing.  step_counts: {batch: steps run at it}.  After a
    packed step of the online-score tracker last_scores is NaN for the slots that did not run.

    aux_format="depth16" (default "rgb8": nothing below exists): image[1] of every pair is the raw (H, W) depth
    frame (numpy uint16, torch uint16, or torch int16 as the bit pattern; host or device) of the RGB frame's size.
    Each slot has a uint16 depth buffer and a depth descriptor in a device table; mmt_depth_prepare_table over
    that table is the first node of the full and of every packed step graph, with an enable byte per slot that
    follows the slot's active flag, and `assign` prepares the slot's first frame eagerly before the template crop.
    The prepared frame is written into the slot's second frame buffer, so the crops, slot_cache, pack and
    online_size work as they do on uploaded frames.

    Failures: a slot whose search crop side falls below 1 (the reference's "Too small bounding
    box.") is released by `track`, and the returned mapping carries the Exception object in place of
    that slot's box; the other slots are not affected."""

    def __init__(self, network, template_factor, template_size, search_factor, search_size, update_intervals,
                 multimodal, online_score=False, use_graph=True, kv_cache=False, slots=1, slot_cache=False,
                 refresh_slots=None, pack=None, online_size=1, max_score_decay=1.0, aux_format="rgb8"):
        self.aux_format = check_aux_format(aux_format)
        # online_size K > 1: count and ring per slot (online_memory_schedule), slot_cache on or off; the step
        # graph reads every slot's valid template rows from the workspace's TL buffer, so slots at different
        # fill levels share one replay.  Not with pack.
        self.online_size, self.max_score_decay = check_online_memory(online_size, max_score_decay, online_score, network)
        self._ring = self.online_size > 1 or self.max_score_decay != 1.0
        if self.online_size > 1 and pack:
            raise ValueError("pack (steps sized to the active slots) is not implemented for online_size > 1")
        if kv_cache:
            raise NotImplementedError("kv_cache is the whole-batch template pass, the batched tracker's template "
                                      "updates are per slot: use slot_cache=True (the per-slot template K/V cache)")
        if int(slots) < 1:
            raise ValueError("slots must be >= 1")
        self.net = network
        self.slots = N = int(slots)
        self.pack = pack_rungs(pack, N)
        self._packs = {}  # rung -> its list, buffers, plan and graph
        self.step_counts = {}
        self.slot_cache = bool(slot_cache)
        self.refresh_slots = min(8, N) if refresh_slots is None else int(refresh_slots)
        if self.slot_cache and not 1 <= self.refresh_slots <= N:
            raise ValueError("refresh_slots must be in 1..slots")
        self._dirty = set()
        self._sc = None
        self.refresh_replays = 0
        self.tf, self.ts, self.sf, self.ss = float(template_factor), int(template_size), float(search_factor), int(search_size)
        self.update_intervals = list(update_intervals)
        self.online_score = bool(online_score)
        self.use_graph = bool(use_graph)
        self.dev = torch.device("cuda", torch.cuda.current_device())
        dev = self.dev
        self.lut = torch.from_numpy(jet_lut().reshape(-1)).to(dev) if multimodal else None
        z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)  # noqa: E731
        self.state = z(N, 4, dt=torch.float64)
        self.template = [z(N, 3, self.ts, self.ts) for _ in range(2)]
        self.online_template = [z(N, 3, self.ts, self.ts) for _ in range(2)]
        if self.online_size > 1:
            self.online_template = [z(N, self.online_size, 3, self.ts, self.ts) for _ in range(2)]
        self.online_count, self.forget_id = [1] * N, [0] * N
        self._counts_dirty = True  # the host counts differ from the runtime's TL buffer
        self.online_max_template = [z(N, 3, self.ts, self.ts) for _ in range(2)]
        self.search = [z(N, 3, self.ss, self.ss) for _ in range(2)]
        self.search_crop = z(N, 2, 4, dt=torch.float64)
        self.tmpl_crop = z(N, 2, 4, dt=torch.float64)
        self.hw = z(N, 2, dt=torch.int32)
        self.active = z(N, dt=torch.uint8)
        self.frame_id = [0] * N
        self.max_pred_score = [-1.0] * N
        self.frames = [None] * N  # per slot [rgb, tir] flat uint8 buffers, at least H * W * 3 bytes
        self._hw = [(0, 0)] * N
        self._active = [False] * N
        self._act = []  # the active slots, ascending
        # crop tables: entry 2 b + m = slot b, modality m.  A zeroed entry (image NULL) is skipped by
        # the kernel.  The template table writes where the tracker's schedule crops: the online
        # template (plain trackers) or the candidate (online-score tracker).
        self._esz = ctypes.sizeof(CropParams)
        self._search_host, self._tmpl_host = (CropParams * (2 * N))(), (CropParams * (2 * N))()
        self._search_tab, self._tmpl_tab = z(2 * N * self._esz, dt=torch.uint8), z(2 * N * self._esz, dt=torch.uint8)
        self._search_enable, self._tmpl_enable = z(2 * N, dt=torch.uint8), z(2 * N, dt=torch.uint8)
        self._tmpl_dst = self.online_max_template if self.online_score else self.online_template
        self._fview = [None] * N  # per slot the (H, W, 3) views of its frame buffers
        if self.aux_format == "depth16":
            # per slot a uint16 depth buffer (kept as int16 bits) and a depth descriptor: entry b prepares slot b's
            # depth frame into its second frame buffer; its enable byte follows the slot's active flag
            self._dbuf, self._dview = [None] * N, [None] * N
            self._dsz = ctypes.sizeof(DepthParams)
            self._depth_host = (DepthParams * N)()
            self._depth_tab = z(N * self._dsz, dt=torch.uint8)
            self._depth_enable = z(N, dt=torch.uint8)
            self._depth_work = z(N, DEPTH_WORK_BYTES, dt=torch.uint8)
        self._readback = [self.state.view(-1), self.search_crop[:, 0, 2]]  # what a step returns to the host
        self._graph = self._plan = self._rt = self._ws = self._ws_tl = None
        self.last_scores = None  # online-score tracker: every slot's sigmoid(score) of the last step
        if self.slot_cache:  # the runtime's refusal, here rather than at the first track
            from .runtime import refuse_cache_with_ce
            refuse_cache_with_ce(getattr(network, "variant", None))

    # ------------------------------------------------------------------ tables and frames
    def _write_entries(self, b):
        """Slot b's four descriptors, from its frame buffers and size, into the device tables."""
        H, W = self._hw[b]
        self._fview[b] = [buf[:H * W * 3].view(H, W, 3) for buf in self.frames[b]]
        for m in range(2):
            im = self._fview[b][m]
            lut = self.lut if m == 1 else None
            self._search_host[2 * b + m] = crop_params(im, self.state[b], self.sf, self.ss, out=self.search[m][b].view(-1),
                                                       crop=self.search_crop[b, m], lut=lut)
            self._tmpl_host[2 * b + m] = crop_params(im, self.state[b], self.tf, self.ts, out=self._tmpl_dst[m][b].view(-1),
                                                     crop=self.tmpl_crop[b, m], lut=lut)
        lo, hi = 2 * b * self._esz, (2 * b + 2) * self._esz
        for host, tab in ((self._search_host, self._search_tab), (self._tmpl_host, self._tmpl_tab)):
            tab[lo:hi].copy_(torch.frombuffer(host, dtype=torch.uint8)[lo:hi])
        self.hw[b].copy_(torch.tensor([H, W], dtype=torch.int32))
        if self.aux_format == "depth16":
            self._dview[b] = self._dbuf[b][:H * W].view(H, W)
            self._depth_host[b] = depth_params(self._dview[b], self._fview[b][1], self._depth_work[b])
            lo, hi = b * self._dsz, (b + 1) * self._dsz
            self._depth_tab[lo:hi].copy_(torch.frombuffer(self._depth_host, dtype=torch.uint8)[lo:hi])

    def _load_frames(self, b, image):
        """Copy slot b's two (H, W, 3) uint8 frames (numpy or torch) into its device buffers; a new
        frame size grows the buffers if needed and rewrites the slot's table entries.  aux_format="depth16":
        the second frame is the raw (H, W) depth frame, copied into the slot's depth buffer; the step graph (or
        `assign`) prepares it into the second frame buffer."""
        depth = None
        if self.aux_format == "depth16":
            H, W, rgb, depth = _split_pair(image)
            ims = [rgb]
        else:
            if not isinstance(image, (list, tuple)) or len(image) != 2:
                raise ValueError("image must be [image_v, image_i]")
            ims = [torch.as_tensor(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x for x in image]
            H, W = ims[0].shape[:2]
            if any(tuple(x.shape) != (H, W, 3) or x.dtype != torch.uint8 for x in ims) or H <= 0 or W <= 0:
                raise ValueError("frames must be two (H, W, 3) uint8 images of the same size")
        if self.frames[b] is None or self.frames[b][0].numel() < H * W * 3:
            self.frames[b] = [torch.empty(H * W * 3, device=self.dev, dtype=torch.uint8) for _ in range(2)]
            if depth is not None:
                self._dbuf[b] = torch.empty(H * W, device=self.dev, dtype=torch.int16)
            self._hw[b] = (0, 0)
        if self._hw[b] != (H, W):
            self._hw[b] = (H, W)
            self._write_entries(b)
        for dst, src in zip(self._fview[b], ims):
            dst.copy_(src, non_blocking=src.device.type == "cuda")
        if depth is not None:
            self._dview[b].copy_(depth, non_blocking=depth.device.type == "cuda")

    def _set_active(self, b, on):
        self._active[b] = bool(on)
        self._act = [i for i in range(self.slots) if self._active[i]]
        self.active[b] = int(on)
        self._search_enable[2 * b:2 * b + 2] = int(on)
        if self.aux_format == "depth16":
            self._depth_enable[b] = int(on)

    def _depth_node(self):
        """aux_format="depth16": the first launches of every step, full or packed: the active slots' depth frames
        prepared into their second frame buffers (an inactive slot's entry is disabled: nothing of it is written)."""
        if self.aux_format != "depth16":
            return []
        return [(LIB.mmt_depth_prepare_table, (self._depth_tab.data_ptr(), self._depth_enable.data_ptr(), self.slots),
                 "track_depth_prepare_table", None)]

    def _crop_templates(self, slots):
        """One table launch: both modalities' template crops of `slots`, each at its slot's state."""
        en = torch.zeros(2 * self.slots, dtype=torch.uint8)
        for b in slots:
            en[2 * b:2 * b + 2] = 1
        self._tmpl_enable.copy_(en)
        check(LIB.mmt_sample_target_table(self._tmpl_tab.data_ptr(), self._tmpl_enable.data_ptr(), 2 * self.slots, self.ts,
                                          torch.cuda.current_stream().cuda_stream), "mmt_sample_target_table")

    # ------------------------------------------------------------------ per-frame plan
    def _slot_state(self, rt):
        """The runtime's refresh state over this tracker's template buffers (built once per runtime)."""
        return rt.slot_cache_workspace(self.slots, self.refresh_slots, self.template, self.online_template)

    def _build_step(self):
        rt = self.net._runtime(self.dev)
        self._rt = rt  # the graph points into this runtime's weights and workspace (see RGBTTrackerCore)
        N = self.slots
        if self.slot_cache:
            self._sc = self._slot_state(rt)
            model_plan = rt.plan_for_inputs(None, None, self.search, run_score_head=self.online_score, part="s")
        else:
            model_plan = rt.plan_for_inputs(self.template, self.online_template, self.search,
                                            run_score_head=self.online_score)
        ws = self._ws = rt.workspace(N)
        plan = self._depth_node()
        plan.append((LIB.mmt_sample_target_table, (self._search_tab.data_ptr(), self._search_enable.data_ptr(), 2 * N, self.ss),
                     "track_sample_target_table", None))
        plan += model_plan
        plan.append((LIB.mmt_track_update_slots, (ws["BOX"].data_ptr(), self.search_crop.data_ptr(), 8, self.state.data_ptr(),
                                                  self.hw.data_ptr(), self.active.data_ptr(), N, self.ss, 10.0),
                     "track_update_slots", None))
        self._plan = plan
        if self.use_graph:
            saved = self.state.clone()  # capture_plan runs the plan once: keep this frame's states
            self._graph = rt.capture_plan(plan)
            self.state.copy_(saved)
        else:
            self._graph = None

    def _build_pack(self, rt, R):
        """Rung R's slot list, batch-R inputs, launch plan and (at its first step) graph."""
        N, dev = self.slots, self.dev
        z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)  # noqa: E731
        pk = {"R": R, "members": None, "graph": None,
              "list": torch.full((R,), -1, device=dev, dtype=torch.int32),
              "search": z(2, R, 3, self.ss, self.ss)}  # one buffer: [modality][row], the packed crop's two strides
        search = [pk["search"][0], pk["search"][1]]
        key = ("pack", N, R)
        if self.slot_cache:
            ws, gather = rt.slot_pack_gather(N, R, pk["list"], key)
            model_plan = rt.plan_for_inputs(None, None, search, run_score_head=self.online_score, part="s", ws_key=key)
        else:
            pk["template"] = [z(R, 3, self.ts, self.ts) for _ in range(2)]
            pk["online_template"] = [z(R, 3, self.ts, self.ts) for _ in range(2)]
            ws, gather = rt.slot_pack_gather(N, R, pk["list"], key, self.template, self.online_template,
                                             pk["template"], pk["online_template"])
            model_plan = rt.plan_for_inputs(pk["template"], pk["online_template"], search,
                                            run_score_head=self.online_score, ws_key=key)
        row = 3 * self.ss * self.ss
        plan = self._depth_node()
        plan.append((LIB.mmt_sample_target_packed, (self._search_tab.data_ptr(), self._search_enable.data_ptr(),
                                                    pk["list"].data_ptr(), R, N, 2, self.ss, pk["search"].data_ptr(), R * row, row),
                     "track_sample_target_packed", None))
        plan += gather
        plan += model_plan
        plan.append((LIB.mmt_track_update_packed, (ws["BOX"].data_ptr(), self.search_crop.data_ptr(), 8, self.state.data_ptr(),
                                                   self.hw.data_ptr(), self.active.data_ptr(), pk["list"].data_ptr(), R, N,
                                                   self.ss, 10.0),
                     "track_update_packed", None))
        pk["ws"], pk["plan"] = ws, plan
        return pk

    def _step(self):
        """Runs one step; returns the packed rung's state, or None after the full step."""
        rt = self.net._runtime(self.dev)
        if (self._plan is not None or self._packs) and rt is not self._rt:
            self._graph = self._plan = None  # weights reloaded: re-plan, re-capture
            self._packs = {}
            if self.slot_cache:  # the new runtime's cache holds none of the templates
                self._dirty.update(self._act)
        R = choose_rung(self.pack, len(self._act)) if self.pack else None
        if R is None:
            if self._plan is None or (self.use_graph and self._graph is None):
                self._build_step()
            pk, graph, plan = None, self._graph, self._plan
        else:
            if self._rt is not rt or (self.slot_cache and self._sc is None):
                self._rt = rt
                if self.slot_cache:
                    self._sc = self._slot_state(rt)
            pk = self._packs.get(R)
            if pk is None:
                pk = self._packs[R] = self._build_pack(rt, R)
            if pk["members"] != self._act:
                pk["list"].copy_(torch.tensor(pack_list(self._act, R), dtype=torch.int32))
                pk["members"] = list(self._act)
        if self.online_size > 1 and (self._counts_dirty or self._ws_tl is not self._ws):
            self._rt.load_online_count(self._ws, self.online_count)  # before the refresh: its staging pass reads them
            self._counts_dirty, self._ws_tl = False, self._ws
        if self._dirty:  # slot cache: template pass of the slots whose templates changed
            self.refresh_replays += self._rt.refresh_template_slots(self._sc, sorted(self._dirty), self.use_graph)
            self._dirty.clear()
        if pk is not None:
            if self.use_graph and pk["graph"] is None:
                saved = self.state.clone()  # capture_plan runs the plan once: keep this frame's states
                pk["graph"] = self._rt.capture_plan(pk["plan"])
                self.state.copy_(saved)
            graph, plan = pk["graph"], pk["plan"]
        if graph is not None:
            graph.replay()
        else:
            self._rt.run_plan(plan)
        B = self.slots if pk is None else pk["R"]
        self.step_counts[B] = self.step_counts.get(B, 0) + 1
        return pk

    # ------------------------------------------------------------------ tracker API
    def active_slots(self):
        return list(self._act)

    def assign(self, slot, image, init_bbox):
        """Start a sequence in `slot`: first frame pair and its box (x, y, w, h)."""
        b = int(slot)
        if not 0 <= b < self.slots:
            raise IndexError("slot %d of %d" % (b, self.slots))
        self._load_frames(b, image)
        if self.aux_format == "depth16":  # eagerly, before the template crop reads the frame
            check(LIB.mmt_depth_prepare(ctypes.byref(self._depth_host[b]), 1, torch.cuda.current_stream().cuda_stream),
                  "mmt_depth_prepare")
        self.state[b].copy_(torch.tensor([float(v) for v in init_bbox], dtype=torch.float64))
        self._crop_templates([b])
        for m in range(2):
            src = self._tmpl_dst[m][b]
            for dst in (self.template, self.online_template, self.online_max_template):
                if dst is not self._tmpl_dst:  # the candidate starts as the template (reference defect D6)
                    if dst is self.online_template and self.online_size > 1:  # slot 0; the others are not read yet
                        dst[m][b].zero_()
                        dst[m][b, 0].copy_(src)
                    else:
                        dst[m][b].copy_(src)
        self.frame_id[b] = 0
        self.max_pred_score[b] = -1.0
        self.online_count[b], self.forget_id[b] = 1, 0
        self._counts_dirty = True
        self._set_active(b, True)
        if self.slot_cache:
            self._dirty.add(b)
        if float(self.tmpl_crop[b, :, 2].min()) < 1:
            self.release(b)
            raise Exception("Too small bounding box.")  # processing_utils.py:36-37

    def release(self, slot):
        """Stop tracking in `slot`: its crops and box update are skipped and its state stays as it is."""
        self._set_active(int(slot), False)
        self._dirty.discard(int(slot))

    def track(self, images):
        """One frame of every active slot.  images: {slot: [image_v, image_i]}, exactly the active
        slots.  Returns {slot: [x, y, w, h]}; a slot that failed (released here) maps to its Exception."""
        act = self._act
        ok = len(images) == len(act)
        for b in act:
            ok = ok and b in images
        if not ok:
            raise ValueError("track needs one frame pair per active slot %s, got %s" % (act, sorted(images)))
        if not act:
            return {}
        for b in act:
            self._load_frames(b, images[b])
            self.frame_id[b] += 1
        pk = self._step()
        N = self.slots
        parts = self._readback
        if self.online_score:
            parts = parts + [torch.sigmoid((self._ws if pk is None else pk["ws"])["SC"].view(-1)).double()]
        vals = torch.cat(parts).tolist()  # the step's one host round trip, for all slots
        if self.online_score and pk is not None:  # the rung's rows back to their slots
            scores = [float("nan")] * N
            for j, b in enumerate(act):
                scores[b] = vals[5 * N + j]
            vals[5 * N:] = scores
        out, crop, promote, writes = {}, [], [], []
        for b in act:
            if vals[4 * N + b] < 1:
                self.release(b)
                out[b] = Exception("Too small bounding box.")  # processing_utils.py:36-37
                continue
            out[b] = vals[4 * b:4 * b + 4]
            score = vals[5 * N + b] if self.online_score else None
            if self._ring:
                c, w, (self.online_count[b], self.forget_id[b], self.max_pred_score[b]) = online_memory_schedule(
                    self.frame_id[b], self.update_intervals, score,
                    (self.online_count[b], self.forget_id[b], self.max_pred_score[b]), self.online_size, self.max_score_decay)
                if c:
                    crop.append(b)
                if w:
                    writes.append((b, w))
                continue
            c, p, self.max_pred_score[b] = template_schedule(self.online_score, self.frame_id[b], self.update_intervals,
                                                             score, self.max_pred_score[b])
            if c:
                crop.append(b)
            if p:
                promote.append((b, p))
        if self.online_score:
            self.last_scores = vals[5 * N:]
        if crop:
            self._crop_templates(crop)
        if self.slot_cache:  # the online template changed: re-crop (plain) or promotion (online score)
            self._dirty.update([b for b, _ in promote] if self.online_score else crop)
        if promote:
            idx = torch.tensor([b for b, _ in promote], device=self.dev)
            twice = [b for b, p in promote if p > 1]
            for m in range(2):
                self.online_template[m][idx] = self.online_max_template[m][idx]
                self.online_max_template[m][idx] = self.template[m][idx]
                if twice:  # a second interval on the same frame promotes the reset candidate
                    i2 = torch.tensor(twice, device=self.dev)
                    self.online_template[m][i2] = self.template[m][i2]
        if writes:  # the ring: per slot the first write takes the candidate, any further one the template
            if self.slot_cache:
                self._dirty.update(b for b, _ in writes)
            self._counts_dirty = True
            for m in range(2):
                for b, w in writes:
                    for j, slot in enumerate(w):
                        src = self.online_max_template if j == 0 else self.template
                        (self.online_template[m][b, slot] if self.online_size > 1 else self.online_template[m][b]).copy_(src[m][b])
                    self.online_max_template[m][b].copy_(self.template[m][b])
        return out


class SequenceBoxes(list):
    """The boxes of one sequence ([x, y, w, h] per frame, the first being init_bbox); `error` is the
    exception that ended the sequence early, or None."""
    error = None


def track_sequences(core, sequences, slots=None):
    """Track every sequence of `sequences` on `core` (an RGBTBatchTrackerCore, or anything with its
    assign / release / track and a `slots` count), keeping the slots full: a slot whose sequence ends
    is released and takes the next one.  sequences: iterable of (name, frames, init_bbox), frames an
    iterable of [image_v, image_i]; the first frame carries init_bbox.  Returns {name: SequenceBoxes}:
    one box per frame; a sequence that failed keeps the boxes up to the failure and the exception in
    `.error` (its slot was released by `core.track`, or never taken when `assign` raised)."""
    n = int(core.slots if slots is None else slots)
    pending = iter(sequences)
    running = {}  # slot -> (name, frame iterator)
    results = {}

    def fill(slot):
        for name, frames, init_bbox in pending:
            it = iter(frames)
            boxes = results[name] = SequenceBoxes()
            first = next(it, None)
            if first is None:
                continue
            try:
                core.assign(slot, first, init_bbox)
            except Exception as e:  # this sequence cannot start; the slot stays free for the next
                boxes.error = e
                continue
            boxes.append([float(v) for v in init_bbox])
            running[slot] = (name, it)
            return

    for slot in range(n):
        fill(slot)
    while running:
        images = {}
        for slot in sorted(running):
            name, it = running[slot]
            frame = next(it, None)
            while frame is None:  # sequence done: free the slot, start the next sequence in it
                core.release(slot)
                del running[slot]
                fill(slot)
                if slot not in running:
                    break
                frame = next(running[slot][1], None)
            if frame is not None:
                images[slot] = frame
        if not images:
            break
        for slot, box in core.track(images).items():
            name = running[slot][0]
            if isinstance(box, Exception):  # core.track released the slot
                results[name].error = box
                del running[slot]
                fill(slot)
            else:
                results[name].append(box)
    return results
