"""Host side of the device JPEG decoder (csrc/jpeg.hip, `ops.decode_jpeg`): the marker parser, the batch type and
the DataLoader collate function.  Pure numpy; Pillow is needed only for a file the device does not decode.

    parse(data)    -> Parsed: the frame, the tables, the scan's place in the file and its segments
    probe(data)    -> (True, "") if the device decodes the file, else (False, reason)
    collate(items) -> the loader's batch with item 0 a JpegBatch (a DataLoader `collate_fn` for
                      `Preprocessor(..., raw=True)`): parsed in the worker, unsupported files decoded there with PIL
    JpegBatch      packed scan bytes, records and the segment table as tensors (pinnable), the host-decoded
                   fallbacks as pixels; `.to(device)`; `ops.decode_jpeg(batch)` gives [N][H][W][3] uint8
    MixedJpegBatch / collate_mixed
                   the same for files of MIXED stored sizes, with the per-image geometry table of
                   csrc/jpeg_mixed.h; `ops.decode_resize_jpeg(batch, (h, w))` gives the dense [N][h][w][3] uint8

The device decodes baseline JPEG (SOF0, 8 bit) with one scan holding all components, one component or three with the
ids 1, 2, 3, luma factors (1,1), (2,1) or (2,2) over chroma (1,1), 8-bit quantisation tables, at most two DC and two
AC tables (ids 0, 1), any restart interval, 8 <= W, 1 <= H, both <= 32768, no Adobe marker with a transform other
than 1.  Everything else — progressive, CMYK / YCCK, other factors, several scans, a file that is not a JPEG, a
narrower image — is decoded on the host and travels as pixels inside the same batch."""
from __future__ import annotations

import io
from typing import NamedTuple, Optional

import numpy as np
import torch

REC_BYTES = 1408              # JPEG_REC_BYTES of csrc/jpeg_entropy.h: int32 header[16], qt[4][64], huff[4][272]
REC_QT, REC_HUFF, HUFF_BYTES = 64, 320, 272
MAX_DIM, MIN_WIDTH = 32768, 8
ST_OK, ST_BAD_CODE, ST_OVERRUN, ST_OUT_OF_BYTES, ST_BAD_RESTART, ST_BAD_GEOM = range(6)
STATUS_TEXT = ("ok", "bad Huffman code", "coefficient index above 63", "ran out of bytes",
               "restart marker missing or wrong", "geometry table inconsistent")
# The chunked route of `ops.decode_jpeg` (csrc/jpeg_chunked.h): many lanes inside one segment.  scan="auto" takes it
# when the batch's longest segment has at least CHUNKED_MIN_BYTES bytes; a lane's chunk has CHUNK_BYTES raw bytes, more
# where a segment would otherwise have more than MAX_CHUNK_LANES chunks.  Both are set from one run on an MI355X
# (profiles/jpeg_chunked_bench.txt, files of 480 x 640): wherever the chunked route wins, 64-byte chunks were as fast as
# 128-byte ones or faster (32 files: 3.23 against 3.25 ms, 1024 files: 14.2 against 15.0 ms) and faster than 256 and
# 512; of the segment sizes measured the chunked route loses to the serial one at 1.5 kB (one restart per MCU row)
# and wins from 6.0 kB on (one per four rows; the longest segment of those files has 6031 bytes).
CHUNK_BYTES = 64
CHUNKED_MIN_BYTES = 6000
MAX_CHUNK_LANES = 1024
SCAN_ROUTES = ("auto", "serial", "chunked")

_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                    13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                    45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
              0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic-coded",
              0xCA: "arithmetic-coded progressive", 0xCB: "arithmetic-coded lossless",
              0xCD: "arithmetic-coded differential", 0xCE: "arithmetic-coded differential progressive",
              0xCF: "arithmetic-coded differential lossless"}


class Parsed(NamedTuple):
    """`reason` is "" when the device decodes the file; otherwise why it does not, and only the fields found up to
    there are set.  record / segments / scan are what one image contributes to a JpegBatch: segments are
    {begin, end} offsets into `scan` (the file's bytes [scan_begin, scan_stop))."""
    reason: str
    height: int = 0
    width: int = 0
    components: tuple = ()          # (id, h, v, tq) per component
    restart_interval: int = 0
    scan_begin: int = 0             # the first entropy-coded byte
    scan_end: int = 0               # the FF of the marker that ends the scan (or the file's length)
    record: Optional[np.ndarray] = None     # uint8 [REC_BYTES]; its segment fields are relative to this image
    segments: Optional[np.ndarray] = None   # int32 [nseg][2]
    scan: Optional[np.ndarray] = None       # uint8, the scan with the two bytes of the marker behind it

    @property
    def device(self) -> bool:
        return not self.reason


def _as_bytes(data) -> np.ndarray:
    if torch.is_tensor(data):
        data = data.numpy()
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def parse(data) -> Parsed:
    b = _as_bytes(data)
    n = int(b.size)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        return Parsed("not a JPEG file")
    qt, huff = {}, {}
    frame = adobe = sos = None
    dri, pos = 0, 2
    H = W = 0
    comps = ()
    scan_begin = scan_end = 0
    while pos + 4 <= n:
        if b[pos] != 0xFF:
            return Parsed("marker expected at byte %d" % pos)
        m = int(b[pos + 1])
        if m == 0xFF:                            # fill byte
            pos += 1
            continue
        if m == 0xD9:
            break
        if m == 0x01 or 0xD0 <= m <= 0xD8:       # no length
            pos += 2
            continue
        L = (int(b[pos + 2]) << 8) | int(b[pos + 3])
        if L < 2 or pos + 2 + L > n:
            return Parsed("truncated in front of the scan")
        seg = b[pos + 4:pos + 2 + L]
        if m == 0xDB and sos is None:
            at = 0
            while at < seg.size:
                if seg[at] >> 4:
                    return Parsed("16-bit quantisation table", H, W, comps)
                if at + 65 > seg.size:
                    return Parsed("truncated quantisation table")
                q = np.zeros(64, np.uint8)
                q[_ZIGZAG] = seg[at + 1:at + 65]
                qt[int(seg[at]) & 15] = q
                at += 65
        elif m == 0xC4 and sos is None:
            at = 0
            while at < seg.size:
                if at + 17 > seg.size:
                    return Parsed("truncated Huffman table")
                cnt = seg[at + 1:at + 17]
                k = int(cnt.sum())
                if k > 256 or at + 17 + k > seg.size or (int(seg[at]) >> 4) > 1:
                    return Parsed("damaged Huffman table")
                huff[(int(seg[at]) >> 4, int(seg[at]) & 15)] = (cnt.copy(), seg[at + 17:at + 17 + k].copy())
                at += 17 + k
        elif m == 0xC0 or m in _SOF_NAMES:
            if frame is not None:
                return Parsed("two frame headers")
            if seg.size < 6 or seg.size < 6 + 3 * int(seg[5]):
                return Parsed("truncated frame header")
            frame = m
            H, W = (int(seg[1]) << 8) | int(seg[2]), (int(seg[3]) << 8) | int(seg[4])
            comps = tuple((int(seg[6 + 3 * i]), int(seg[7 + 3 * i]) >> 4, int(seg[7 + 3 * i]) & 15,
                           int(seg[8 + 3 * i])) for i in range(int(seg[5])))
            if m != 0xC0:
                return Parsed(_SOF_NAMES[m], H, W, comps)
            if seg[0] != 8:
                return Parsed("%d-bit samples" % int(seg[0]), H, W, comps)
        elif m == 0xDD and seg.size >= 2 and sos is None:
            dri = (int(seg[0]) << 8) | int(seg[1])
        elif m == 0xEE and seg.size >= 12 and bytes(seg[:5]) == b"Adobe":
            adobe = int(seg[11])
        elif m == 0xDA:
            if sos is not None:
                return Parsed("several scans", H, W, comps)
            if frame is None:
                return Parsed("scan in front of the frame header")
            ns = int(seg[0]) if seg.size else 0
            if seg.size < 4 + 2 * ns:
                return Parsed("truncated scan header")
            if ns != len(comps):
                return Parsed("several scans", H, W, comps)
            sos = ([(int(seg[1 + 2 * i]), int(seg[2 + 2 * i]) >> 4, int(seg[2 + 2 * i]) & 15) for i in range(ns)],
                   int(seg[1 + 2 * ns]), int(seg[2 + 2 * ns]), int(seg[3 + 2 * ns]))
            scan_begin = pos + 2 + L
            # the scan ends at the first FF that is neither stuffed (FF 00) nor a restart marker (FF D0..D7)
            ff = np.flatnonzero(b[scan_begin:n - 1] == 0xFF) + scan_begin
            nxt = b[ff + 1]
            ends = ff[(nxt != 0) & ((nxt < 0xD0) | (nxt > 0xD7))]
            scan_end = int(ends[0]) if ends.size else n
            pos = scan_end
            continue
        pos += 2 + L
    if frame is None or sos is None:
        return Parsed("no frame or no scan", H, W, comps)

    # ---- what the device takes ---------------------------------------------------------------------------------
    def no(reason):
        return Parsed(reason, H, W, comps, dri, scan_begin, scan_end)
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        return no("size %d x %d outside [1, %d]" % (H, W, MAX_DIM))
    if W < MIN_WIDTH:
        return no("narrower than %d pixels" % MIN_WIDTH)
    if len(comps) not in (1, 3):
        return no("%d components (CMYK / YCCK)" % len(comps))
    if adobe is not None and adobe != 1:
        return no("Adobe marker with transform %d" % adobe)
    factors = tuple((h, v) for _, h, v, _ in comps)
    if len(comps) == 3:
        if tuple(c[0] for c in comps) != (1, 2, 3):
            return no("component ids %s, not 1, 2, 3" % (tuple(c[0] for c in comps),))
        if factors[0] not in ((1, 1), (2, 1), (2, 2)) or factors[1:] != ((1, 1), (1, 1)):
            return no("sampling factors %s" % (factors,))
    elif factors[0] != (1, 1):
        return no("sampling factors %s" % (factors,))
    scomps, ss, se, ahal = sos
    if (ss, se, ahal) != (0, 63, 0):
        return no("spectral selection or successive approximation in the scan header")
    if tuple(c[0] for c in scomps) != tuple(c[0] for c in comps):
        return no("scan components in another order")
    for _, td, ta in scomps:
        if td > 1 or ta > 1:
            return no("Huffman table id above 1")
        if (0, td) not in huff or (1, ta) not in huff:
            return no("Huffman table missing")
    for c in comps:
        if c[3] > 3 or c[3] not in qt:
            return no("quantisation table missing")
    rst = ff[(nxt >= 0xD0) & (nxt <= 0xD7) & (ff < scan_end)]
    if dri == 0 and rst.size:
        return no("restart markers without a restart interval")

    # ---- the record and the segments -----------------------------------------------------------------------------
    hs, vs = factors[0] if len(comps) == 3 else (1, 1)
    total = -(-W // (8 * hs)) * -(-H // (8 * vs))
    want = -(-total // dri) if dri else 1
    status = ST_OK
    if rst.size + 1 != want or not np.array_equal(b[rst + 1], 0xD0 + (np.arange(rst.size) & 7)):
        status = ST_BAD_RESTART
        rst = rst[:want - 1]
    stop = min(scan_end + 2, n)
    segs = np.empty((rst.size + 1, 2), np.int32)
    segs[0, 0], segs[1:, 0] = 0, rst + 2 - scan_begin
    segs[:-1, 1], segs[-1, 1] = rst - scan_begin, scan_end - scan_begin
    rec = np.zeros(REC_BYTES, np.uint8)
    hdr = rec[:64].view(np.int32)
    hdr[0], hdr[1], hdr[2] = len(comps), hs, vs
    for i, (c, (_, td, ta)) in enumerate(zip(comps, scomps)):
        hdr[3 + i], hdr[6 + i], hdr[9 + i] = c[3], td, ta
    hdr[12], hdr[13], hdr[14], hdr[15] = dri, 0, segs.shape[0], status
    for t, q in qt.items():
        if t <= 3:
            rec[REC_QT + 64 * t:REC_QT + 64 * t + 64] = q
    for (tc, th), (cnt, vals) in huff.items():
        if th <= 1:
            at = REC_HUFF + HUFF_BYTES * (2 * tc + th)
            rec[at:at + 16] = cnt
            rec[at + 16:at + 16 + vals.size] = vals
    return Parsed("", H, W, comps, dri, scan_begin, scan_end, rec, segs, b[scan_begin:stop])


def probe(data):
    """(True, "") if the device decodes this file, else (False, why not)."""
    p = parse(data)
    return p.device, p.reason


def decode_on_host(data) -> np.ndarray:
    """The fallback: `Image.open(...).convert('RGB')` of the file's bytes, [H][W][3] uint8."""
    from PIL import Image      # imported on first use: only an unsupported file needs Pillow
    with Image.open(io.BytesIO(_as_bytes(data).tobytes())) as im:
        return np.asarray(im.convert("RGB"))


def plane_blocks(H, W):
    """8 x 8 blocks of one component plane of an H x W image in the decoder's workspace, padded to whole 16 x 16 MCUs
    (jpeg_blocks_across of csrc/jpeg_entropy.h per axis); ints or numpy arrays."""
    return (2 * ((W + 15) // 16)) * (2 * ((H + 15) // 16))


class _Batch:
    """What JpegBatch and MixedJpegBatch share: N images and the tensors `_TENSORS` names, moved and pinned together.
    A copy is made through `type(self)` without calling `__init__`, so a subclass keeps its own constructor."""

    _TENSORS = ()

    def __len__(self):
        return self.n

    def _map(self, fn):
        out = type(self).__new__(type(self))
        out.__dict__.update(self.__dict__)
        for name in self._TENSORS:
            setattr(out, name, fn(getattr(self, name)))
        return out

    def to(self, device, non_blocking=False):
        return self._map(lambda t: t.to(device, non_blocking=non_blocking))

    def cuda(self, device=None, non_blocking=False):
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device) \
            if not isinstance(device, torch.device) else device
        return self.to(dev, non_blocking=non_blocking)

    def pin_memory(self):
        return self._map(lambda t: t.pin_memory() if t.numel() else t)

    def is_pinned(self):
        return all(getattr(self, name).is_pinned() for name in self._TENSORS if getattr(self, name).numel())


class _Files(NamedTuple):
    """What `_walk_files` gathers from the files of a batch."""
    scan: torch.Tensor          # uint8, the device-decoded images' scans back to back
    records: torch.Tensor       # uint8 [Nd][REC_BYTES], header word 13 patched to the image's first segment
    segments: torch.Tensor      # int32 [S][2], offsets into `scan`
    max_segments: int
    max_segment_bytes: int
    dev_index: torch.Tensor     # int64: batch positions of the device-decoded images
    host_index: torch.Tensor    # int64: of the host-decoded ones
    host_pixels: list           # numpy uint8 [H][W][3] per host-decoded image
    reasons: list
    sizes: list                 # (H, W) per image


def _walk_files(files, what) -> _Files:
    """Parse the files of a batch (bytes, numpy or 1-D uint8 tensors) for the batch class named `what`: the device's
    share packed, the others decoded on the host."""
    files = list(files)
    if not files:
        raise ValueError(f"{what}: an empty batch")
    scans, recs, segs, dev_idx, host_idx, host_px, reasons, sizes = [], [], [], [], [], [], [], []
    at = nseg = max_seg = max_bytes = 0
    for i, f in enumerate(files):
        p = parse(f)
        reasons.append(p.reason)
        if p.device:
            if at + p.scan.size >= 1 << 31:
                raise ValueError(f"{what}: more than 2^31 scan bytes in one batch (at image {i})")
            rec, sg = p.record.copy(), p.segments + np.int32(at)
            rec[:64].view(np.int32)[13] = nseg
            scans.append(p.scan), recs.append(rec), segs.append(sg), dev_idx.append(i)
            at, nseg, max_seg = at + p.scan.size, nseg + sg.shape[0], max(max_seg, sg.shape[0])
            max_bytes = max(max_bytes, int((sg[:, 1] - sg[:, 0]).max()))
            sizes.append((p.height, p.width))
        else:
            px = np.ascontiguousarray(decode_on_host(f))
            host_idx.append(i), host_px.append(px)
            sizes.append(px.shape[:2])
    t = torch.from_numpy
    return _Files(t(np.concatenate(scans)) if scans else torch.empty(0, dtype=torch.uint8),
                  t(np.stack(recs)) if recs else torch.empty((0, REC_BYTES), dtype=torch.uint8),
                  t(np.concatenate(segs)) if segs else torch.empty((0, 2), dtype=torch.int32),
                  max_seg, max_bytes, torch.tensor(dev_idx, dtype=torch.int64),
                  torch.tensor(host_idx, dtype=torch.int64), host_px, reasons, sizes)


class JpegBatch(_Batch):
    """N stored images of one size H x W on their way to `ops.decode_jpeg`.  Those the device decodes (at the batch
    positions `dev_index`) travel as `scan` (uint8, their scans back to back), `records` (uint8 [Nd][REC_BYTES]) and
    `segments` (int32 [S][2], offsets into `scan`); the others (`host_index`) were decoded on the host and travel as
    `host_pixels` (uint8 [Nh][H][W][3]).  `reasons[i]` says why image i was decoded on the host ("" otherwise).
    `max_segment_bytes`: the longest segment, which chooses the route of `ops.decode_jpeg(scan="auto")`."""

    def __init__(self, n, height, width, scan, records, segments, max_segments, dev_index, host_index, host_pixels,
                 reasons, max_segment_bytes=0):
        self.n, self.height, self.width = int(n), int(height), int(width)
        self.scan, self.records, self.segments = scan, records, segments
        self.max_segments = int(max_segments)
        self.max_segment_bytes = int(max_segment_bytes)
        self.dev_index, self.host_index, self.host_pixels = dev_index, host_index, host_pixels
        self.reasons = tuple(reasons)

    _TENSORS = ("scan", "records", "segments", "dev_index", "host_index", "host_pixels")

    @property
    def shape(self):
        return (self.n, self.height, self.width, 3)

    @property
    def is_cuda(self):
        return self.scan.is_cuda or self.host_pixels.is_cuda

    @property
    def device(self):
        return self.scan.device

    @classmethod
    def from_files(cls, files) -> "JpegBatch":
        """files: the bytes of N files (bytes, numpy or 1-D uint8 tensors) of one stored size; ValueError for a mix of
        sizes (a batch of one is always fine)."""
        f = _walk_files(files, "JpegBatch")
        if len(set(f.sizes)) != 1:
            raise ValueError(f"JpegBatch: images of mixed stored sizes {sorted(set(f.sizes))} in one batch (use a "
                             f"batch size of 1 or a loader that groups them)")
        H, W = f.sizes[0]
        host_pixels = torch.from_numpy(np.stack(f.host_pixels)) if f.host_pixels else \
            torch.empty((0, H, W, 3), dtype=torch.uint8)
        return cls(len(f.sizes), H, W, f.scan, f.records, f.segments, f.max_segments, f.dev_index, f.host_index,
                   host_pixels, f.reasons, f.max_segment_bytes)


# ---- batches of mixed stored sizes (csrc/jpeg_mixed.h, csrc/jpeg.hip) ------------------------------------------------
GEOM_INTS = 8                 # JPEG_MIX_GEOM_INTS: H, W, coefficient base, plane base, pixel offset low / high, 0, 0
PIX_ALIGN = 64                # JPEG_MIX_PIX_ALIGN: every image of the packed pixels starts on a multiple of it
MAX_SHRINK = 16               # RS_MAX_SCALE of csrc/resize_tables.h: the largest stored / target size per axis


def mixed_layout(sizes):
    """jpeg_mixed_layout of csrc/jpeg_mixed.h in numpy (a loader's worker lays its batch out without loading the
    library; tests/test_jpeg_mixed_cpu.py holds it to `oibl_jpeg_mixed_layout`): sizes int [N][2] = {H, W} ->
    (geom int32 [N][GEOM_INTS], totals): the images back to back in the coefficients, the sample planes and the packed
    pixels.  totals = (coefficient bytes, plane bytes, packed pixel bytes, largest Bw * Bh, largest H, largest W)."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    N = sizes.shape[0]
    if not 1 <= N <= 65535:
        raise ValueError(f"mixed_layout: N = {N} must be in [1, 65535]")
    bad = np.flatnonzero((sizes < 1).any(1) | (sizes > MAX_DIM).any(1))
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"mixed_layout: image {i} is {sizes[i, 0]} x {sizes[i, 1]}, every side must be in "
                         f"[1, {MAX_DIM}]")
    H, W = sizes[:, 0], sizes[:, 1]
    bb = plane_blocks(H, W)
    blocks = np.concatenate([[0], np.cumsum(3 * bb)])
    if blocks[-1] >= 1 << 31:
        raise ValueError(f"mixed_layout: 2^31 coefficient blocks or more at image "
                         f"{int(np.argmax(blocks[1:] >= 1 << 31))}")
    pix = np.zeros(N, np.int64)
    end = 0
    for i in range(N):
        pix[i] = -(-end // PIX_ALIGN) * PIX_ALIGN
        end = int(pix[i] + 3 * H[i] * W[i])
        if end >= 1 << 40:
            raise ValueError(f"mixed_layout: 2^40 packed pixel bytes or more at image {i}")
    geom = np.zeros((N, GEOM_INTS), np.int32)
    geom[:, 0], geom[:, 1], geom[:, 2], geom[:, 3] = H, W, blocks[:-1], blocks[:-1]
    geom[:, 4] = (pix & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    geom[:, 5] = pix >> 32
    return geom, (int(blocks[-1]) * 128, int(blocks[-1]) * 64, end, int(bb.max()), int(H.max()), int(W.max()))


def geom_pixel_offsets(geom) -> np.ndarray:
    """int64 [N]: every image's byte offset in the packed pixels, from a geometry table (numpy or a host tensor)."""
    g = geom.numpy() if torch.is_tensor(geom) else np.asarray(geom)
    return g[:, 4].astype(np.int64) & 0xFFFFFFFF | g[:, 5].astype(np.int64) << 32


def check_shrink(sizes, target, what="MixedJpegBatch") -> None:
    """ValueError for the first image a resize to target = (h, w) would shrink by more than MAX_SHRINK on an axis."""
    h2, w2 = int(target[0]), int(target[1])
    if h2 < 1 or w2 < 1:
        raise ValueError(f"{what}: the target size must be positive, got {h2} x {w2}")
    for i, (h, w) in enumerate(np.asarray(sizes).reshape(-1, 2).tolist()):
        if h > MAX_SHRINK * h2 or w > MAX_SHRINK * w2:
            raise ValueError(f"{what}: image {i} is {h} x {w}: a resize to {h2} x {w2} shrinks an axis by more than "
                             f"the limit of {MAX_SHRINK}")


class MixedJpegBatch(_Batch):
    """N stored images of ANY sizes on their way to `ops.decode_resize_jpeg` / `ops.decode_jpeg_mixed`.  As in a
    JpegBatch the images the device decodes (batch positions `dev_index`) travel as `scan`, `records` and `segments`,
    the others (`host_index`; `reasons[i]` says why) as pixels decoded on the host: `host_pixels`, ONE packed uint8
    tensor, image j of them at `host_offsets[j]` — the flow never fails because of a file's format.
      sizes       int32 [N][2] = {H, W}, always on the host (the C calls size their grids and tables from it)
      geom        int32 [N][GEOM_INTS]: the layout of all N images (`mixed_layout`): where image i lies in the packed
                  pixel buffer of `totals[2]` bytes that the decoder writes and the resize reads; `geom_host` is its
                  copy that stays on the host (numpy)
      dev_geom    int32 [Nd][GEOM_INTS]: the rows of the device-decoded images as `oibl_jpeg_decode_mixed` takes
                  them — their coefficient and plane bases from a layout of those images alone (`dev_totals`), their
                  pixel offsets from `geom`
    `max_segments`, `max_segment_bytes`: as for JpegBatch."""

    _TENSORS = ("scan", "records", "segments", "dev_index", "host_index", "host_pixels", "geom", "dev_geom")

    def __init__(self, n, sizes, geom, totals, dev_geom, dev_totals, scan, records, segments, max_segments, dev_index,
                 host_index, host_pixels, host_offsets, reasons, max_segment_bytes=0):
        self.n = int(n)
        self.sizes, self.geom, self.totals = sizes, geom, tuple(int(v) for v in totals)
        # the host's copy of the table (numpy, never moved): where the views and the host-decoded slots lie
        self.geom_host = geom.cpu().numpy().copy()
        self.dev_geom, self.dev_totals = dev_geom, tuple(int(v) for v in dev_totals)
        self.scan, self.records, self.segments = scan, records, segments
        self.max_segments, self.max_segment_bytes = int(max_segments), int(max_segment_bytes)
        self.dev_index, self.host_index = dev_index, host_index
        self.host_pixels, self.host_offsets = host_pixels, tuple(int(v) for v in host_offsets)
        self.reasons = tuple(reasons)

    @property
    def is_cuda(self):
        return self.geom.is_cuda

    @property
    def device(self):
        return self.geom.device

    @property
    def uniform(self) -> bool:
        """Do all images have one stored size?"""
        return bool((self.sizes == self.sizes[0]).all())

    @classmethod
    def from_files(cls, files, target=None) -> "MixedJpegBatch":
        """files: the bytes of N files (bytes, numpy or 1-D uint8 tensors) of any stored sizes.  target = (h, w): the
        size the batch will be resized to; an image beyond the resize's per-axis shrink limit then raises ValueError
        here, in the loader's worker (without it the device call raises).  A file with a side above MAX_DIM = 32768
        — only a host-decoded one can have it, a PNG for instance — is a ValueError as well: neither the layout nor
        the resize takes it, as `ops.resize_u8` does not."""
        f = _walk_files(files, "MixedJpegBatch")
        sizes = np.asarray(f.sizes, np.int32).reshape(-1, 2)
        if target is not None:
            check_shrink(sizes, target)
        geom, totals = mixed_layout(sizes)
        dev_idx = f.dev_index.tolist()
        if dev_idx:
            dev_geom, dev_totals = mixed_layout(sizes[dev_idx])
            dev_geom[:, 4:6] = geom[dev_idx, 4:6]
            dev_totals = dev_totals[:2] + (totals[2],) + dev_totals[3:]
        else:
            dev_geom, dev_totals = np.zeros((0, GEOM_INTS), np.int32), (0, 0, totals[2], 0, 0, 0)
        t = torch.from_numpy
        host_px = [px.reshape(-1) for px in f.host_pixels]
        return cls(len(sizes), t(sizes), t(geom), totals, t(dev_geom), dev_totals, f.scan, f.records, f.segments,
                   f.max_segments, f.dev_index, f.host_index,
                   t(np.concatenate(host_px)) if host_px else torch.empty(0, dtype=torch.uint8),
                   np.concatenate([[0], np.cumsum([p.size for p in host_px])]).astype(np.int64), f.reasons,
                   f.max_segment_bytes)


def scan_route(input_decode) -> str:
    """The `scan` of `ops.decode_jpeg` an `input_decode` argument asks for: a route's name is itself, anything else
    that is true is "auto"."""
    if not isinstance(input_decode, str):
        return "auto"
    if input_decode in SCAN_ROUTES:
        return input_decode
    raise ValueError(f"input_decode must be True or one of {SCAN_ROUTES}, not {input_decode!r}")


def _collate(items, make):
    from torch.utils.data import default_collate
    first = items[0]
    if torch.is_tensor(first) or isinstance(first, (bytes, bytearray, np.ndarray)):
        return make(items)
    rest = default_collate([tuple(it[1:]) for it in items]) if len(first) > 1 else []
    return [make([it[0] for it in items])] + list(rest)


def collate(items):
    """DataLoader `collate_fn` for a dataset whose item 0 is a file's bytes (`Preprocessor(..., raw=True)`): item 0 of
    the batch is a JpegBatch, the other fields are collated as usual."""
    return _collate(items, JpegBatch.from_files)


def collate_mixed(items, target=None):
    """`collate` for files of mixed stored sizes: item 0 of the batch is a MixedJpegBatch, the other fields are
    collated as usual.  target = (h, w), the size of the resize behind the decoder, makes an image beyond the resize's
    shrink limit a ValueError in the worker: `collate_fn=functools.partial(jpeg.collate_mixed, target=(480, 640))`."""
    return _collate(items, lambda files: MixedJpegBatch.from_files(files, target=target))


def collate_tuples(items, target=None):
    """DataLoader `collate_fn` for a TUPLE sampler over `Preprocessor(..., raw=True)` (the training loaders): `items`
    are B tuples, each a list of N items (bytes, fname, pid, x, y).  Item 0 of the result is ONE MixedJpegBatch of the
    B * N files in tuple-major order (file n of tuple b at b * N + n) with the attribute `tuples = (B, N)` — always a
    mixed batch, whether or not the stored sizes agree — for a trainer whose `augment` starts with
    `augment.DecodeJpeg`.  The other fields follow as `default_collate` collates them for such a loader: one entry per
    tuple position n, the list [fnames (B), pids [B], x [B], y [B]].  target = (h, w) as for `collate_mixed`: an image
    beyond the resize's shrink limit is a ValueError in the worker.  Tuples of unequal length are a ValueError."""
    from torch.utils.data import default_collate
    items = [list(t) for t in items]
    if not items or not items[0]:
        raise ValueError("collate_tuples: an empty batch")
    B, N = len(items), len(items[0])
    for b, t in enumerate(items):
        if len(t) != N:
            raise ValueError(f"collate_tuples: tuple {b} has {len(t)} images, tuple 0 has {N}: the tuples of a batch "
                             f"must have one length")
    batch = MixedJpegBatch.from_files([it[0] for t in items for it in t], target=target)
    batch.tuples = (B, N)
    rest = default_collate([[tuple(it[1:]) for it in t] for t in items]) if len(items[0][0]) > 1 else []
    return [batch] + list(rest)


def tuple_names(batch):
    """The file names of a `collate_tuples` batch in the order of its MixedJpegBatch (b * N + n), or None."""
    B, N = batch[0].tuples
    rest = batch[1:]
    if len(rest) != N or not all(isinstance(r, (list, tuple)) and r and len(r[0]) == B for r in rest):
        return None
    return [str(rest[n][0][b]) for b in range(B) for n in range(N)]
