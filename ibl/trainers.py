"""Training loops with the reference's interface (ibl/trainers.py): `Trainer` (NetVLAD's triplet loss, SARE) and
`SFRSTrainer` (self-supervised region similarities), over the differentiable device path of openibl_amd.

What differs from the reference, and why:
  * the model call is `model.forward_train(inputs, train_layers=...)`: `forward()` of this package's models is the
    gradient-free inference path.  `train_layers` is read off the model: None when no backbone parameter requires a
    gradient (the "train only the VLAD layer" setting), `base_model.train_layers` otherwise — 'conv5' trains on the
    device, deeper settings raise NotImplementedError from `forward_train` (the gradient stops at pool4);
  * every loss is one fused call (ops.tuple_loss, ops.soft_label_loss: two launches forward, one backward, fp64
    inside) instead of a chain of torch launches; from SFRS generation 1 on, the hard loss of the whole batch is ONE
    such call behind one argmax and one gather, not a Python loop over the tuples;
  * an unknown loss_type raises ValueError (the reference's `assert ("Unknown loss function")` never fires);
  * `vlad=False` (max-pooled features) raises NotImplementedError: pool_x carries no graph here;
  * single rank: no gradient all-reduce is added (the reference leaves that to DistributedDataParallel);
  * `augment` (extension, off by default): with an openibl_amd.augment.ColorJitter set, the loader delivers raw uint8
    tuples (`get_transformer_train(..., as_uint8=True)`) and `_parse_data` jitters and normalises them on the device —
    the reference's ColorJitter runs inside its host transform;
  * training from the files' bytes (extension): a loader over `Preprocessor(..., raw=True)` with
    `collate_fn=openibl_amd.jpeg.collate_tuples` hands over ONE MixedJpegBatch per batch, and `augment` =
    Compose(DecodeJpeg(), ColorJitter(..., out='uint8'), Resize(h, w)) decodes, jitters and resizes it on the device in
    the reference's order, for any mix of stored sizes.  The decoder's per-image status is read right behind the
    iteration's `loss.item()` (it travels to pinned memory with the chain: no further synchronisation) and a damaged
    file raises RuntimeError with its name.  `prefetch=True` (off by default) runs that chain for batch i + 1 on a
    side stream while batch i trains.
The loop itself — meters, one `loss.item()` synchronisation per iteration, the printed line — is the reference's."""
from __future__ import annotations

import collections
import time

import torch
import torch.distributed as dist

from openibl_amd import ops

from .utils.meters import AverageMeter

LOSS_TYPES = ("triplet", "sare_ind", "sare_joint")


def _unwrap(model):
    """The model inside a `.module` container (DataParallel / DistributedDataParallel)."""
    return model.module if hasattr(model, "module") and not hasattr(model, "forward_train") else model


def _train_layers(model):
    """None when the whole backbone is frozen, `base_model.train_layers` otherwise."""
    base = _unwrap(model).base_model
    if not any(p.requires_grad for p in base.parameters()):
        return None
    return base.train_layers


def _rank() -> int:
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _check_loss_type(loss_type):
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"unknown loss_type {loss_type!r}: one of {LOSS_TYPES}")


def _stack_tuples(inputs):
    """A loader batch (one entry per tuple position, each `(images [B][C][H][W], ...)`) -> [B][N][C][H][W]."""
    return torch.stack([item[0] for item in inputs]).permute(1, 0, 2, 3, 4)


def _augment_tuples(augment, imgs, gpu):
    """imgs [B][N][H][W][3] uint8 on the host (the loader's raw tuples, `get_transformer_train(..., as_uint8=True)`)
    -> [B][N][3][H'][W'] float32 on the device: the bytes cross as they are, and `augment` (an
    openibl_amd.augment.ColorJitter: [n][H][W][3] uint8 -> [n][3][H][W] float32; or a Compose of it with an
    openibl_amd.augment.Resize behind it, which hands back the target size H' x W') jitters every image on its own."""
    if imgs.dtype != torch.uint8 or imgs.dim() != 5 or imgs.shape[-1] != 3:
        raise ValueError(f"a trainer with `augment` set takes uint8 tuples [B][N][H][W][3] from the loader "
                         f"(get_transformer_train(..., as_uint8=True)), got {imgs.dtype} {tuple(imgs.shape)}")
    B, N, H, W, _ = imgs.shape
    out = augment(imgs.contiguous().cuda(gpu).view(B * N, H, W, 3))
    return out.view(B, N, 3, out.shape[-2], out.shape[-1])


def _is_file_tuples(inputs):
    """Is a loader batch what `openibl_amd.jpeg.collate_tuples` makes: item 0 a MixedJpegBatch with `tuples` set?"""
    from openibl_amd.jpeg import MixedJpegBatch
    return isinstance(inputs, (list, tuple)) and len(inputs) > 0 and isinstance(inputs[0], MixedJpegBatch) and \
        getattr(inputs[0], "tuples", None) is not None


def _file_chain(augment):
    """ValueError unless `augment` is the chain a batch of file bytes needs."""
    from openibl_amd.augment import Compose, DecodeJpeg, Resize
    if isinstance(augment, Compose) and isinstance(augment.stages[0], DecodeJpeg):
        last = augment.stages[-1]
        if isinstance(last, Resize) and not last.keep_aspect and last.out == "float":
            return augment
    raise ValueError(f"a loader batch of file bytes (openibl_amd.jpeg.collate_tuples) needs `augment` to be an "
                     f"openibl_amd.augment.Compose that starts with DecodeJpeg and ends with a Resize without "
                     f"keep_aspect and with out='float' — Compose(DecodeJpeg(), ColorJitter(..., out='uint8'), "
                     f"Resize(height, width)) — got {augment!r}")


def _decode_tuples(augment, inputs, gpu, pending):
    """A `jpeg.collate_tuples` batch (host, pinned or not) -> [B][N][3][H'][W'] float32 on the device, computed on the
    current stream: decode, jitter in place at the stored sizes, resize.  Nothing is read back: the decoder's statuses
    follow the chain into pinned memory and are appended to `pending` with the file names, for `_check_files`."""
    from openibl_amd.jpeg import tuple_names
    chain = _file_chain(augment)
    B, N = inputs[0].tuples
    out = chain(inputs[0].cuda(gpu, non_blocking=True))
    status = chain.stages[0].last_status
    host = torch.empty(status.numel(), dtype=torch.int32).pin_memory()
    host.copy_(status, non_blocking=True)
    pending.append((host, tuple_names(inputs)))
    return out.view(B, N, 3, out.shape[-2], out.shape[-1])


def _check_files(pending):
    """The statuses of the oldest batch `_decode_tuples` left behind, read where the stream that used the batch has
    been drained (behind `loss.item()`); RuntimeError lists the damaged files."""
    if not pending:
        return
    from openibl_amd.jpeg import STATUS_TEXT
    host, names = pending.popleft()
    bad = [f"{names[i] if names is not None else f'item {i}'} ({STATUS_TEXT[min(int(s), len(STATUS_TEXT) - 1)]})"
           for i, s in enumerate(host.tolist()) if s]
    if bad:
        pending.clear()
        raise RuntimeError(f"training input: {len(bad)} damaged JPEG file(s): " + ", ".join(bad))


class _Prefetch(object):
    """`parse(data_loader.next())` of batch i + 1 on a side stream while batch i trains (the trainers' opt-in
    `prefetch=True`).  `issue()` enqueues the next batch's input chain — copies, decode, jitter, resize — on the side
    stream (its own `ops.workspace` scratch: those buffers are per stream) and records an event; `take()` makes the
    current stream wait for that event and hands the tensors over (`record_stream`: they were allocated on the side
    stream and are read on this one, as openibl_amd.extract.EagerLanes hands its inputs to a lane).  The host runs
    the batches in order, so the jitter draws what it draws without prefetch."""

    def __init__(self, parse, data_loader, count, gpu):
        self.parse, self.loader, self.left = parse, data_loader, count
        self.device = torch.device("cuda", torch.cuda.current_device() if gpu is None else gpu)
        self.side = torch.cuda.Stream(device=self.device)
        self.ready = None
        self.issue()

    def issue(self):
        if self.left <= 0:
            return
        self.left -= 1
        with torch.cuda.stream(self.side):
            out = self.parse(self.loader.next())
            ev = torch.cuda.Event()
            ev.record(self.side)
        self.ready = (out, ev)

    def take(self):
        out, ev = self.ready
        self.ready = None
        main = torch.cuda.current_stream(self.device)
        main.wait_event(ev)
        for t in (out if isinstance(out, (tuple, list)) else (out,)):
            t.record_stream(main)
        return out


class Trainer(object):
    """Training module for NetVLAD (CVPR'16, loss_type='triplet') and SARE (ICCV'19, loss_type='sare_ind' or
    'sare_joint').  `model` is an EmbedNet (possibly inside a `.module` container) on the device."""

    def __init__(self, model, margin=0.3, gpu=None, temp=0.07, augment=None, prefetch=False):
        super(Trainer, self).__init__()
        self.model = model
        self.gpu = gpu
        self.margin = margin
        self.temp = temp
        # None: the loader delivers normalised float tuples (the reference's flow); an
        # openibl_amd.augment.ColorJitter: it delivers raw uint8 tuples, jittered and normalised on the device; a
        # Compose that starts with DecodeJpeg: it delivers the files' bytes (jpeg.collate_tuples)
        self.augment = augment
        self.prefetch = prefetch                    # True: batch i + 1's input chain runs on a side stream
        self._files = collections.deque()           # statuses of the file batches not yet checked

    def train(self, epoch, sub_id, data_loader, optimizer, train_iters,
              print_freq=1, vlad=True, loss_type='triplet'):
        _check_loss_type(loss_type)
        self.model.train()

        batch_time, data_time, losses = AverageMeter(), AverageMeter(), AverageMeter()
        end = time.time()
        data_loader.new_epoch()

        self._files.clear()
        ahead = _Prefetch(self._parse_data, data_loader, train_iters, self.gpu) if self.prefetch else None
        for i in range(train_iters):
            inputs = ahead.take() if ahead else self._parse_data(data_loader.next())
            data_time.update(time.time() - end)

            loss = self._forward(inputs, vlad, loss_type)
            if ahead:
                ahead.issue()
            losses.update(loss.item())
            _check_files(self._files)

            optimizer.zero_grad()
            loss.backward()
            optimizer.step()

            batch_time.update(time.time() - end)
            end = time.time()

            if (i + 1) % print_freq == 0 and _rank() == 0:
                print('Epoch: [{}-{}][{}/{}]\t'
                      'Time {:.3f} ({:.3f})\t'
                      'Data {:.3f} ({:.3f})\t'
                      'Loss {:.3f} ({:.3f})'
                      .format(epoch, sub_id, i + 1, train_iters,
                              batch_time.val, batch_time.avg,
                              data_time.val, data_time.avg,
                              losses.val, losses.avg))

    def _parse_data(self, inputs):
        # [B][tuple size][C][H][W]
        if _is_file_tuples(inputs):
            return _decode_tuples(self.augment, inputs, self.gpu, self._files)
        if self.augment is not None:
            return _augment_tuples(self.augment, _stack_tuples(inputs), self.gpu)
        return _stack_tuples(inputs).cuda(self.gpu)

    def _forward(self, inputs, vlad, loss_type):
        _check_loss_type(loss_type)
        B, N, C, H, W = inputs.size()
        if not vlad:
            raise NotImplementedError("Trainer: vlad=False trains on the max-pooled features, and pool_x of "
                                      "EmbedNet.forward_train carries no autograd graph (the global max-pool has no "
                                      "backward on the device); train on the VLAD descriptor (vlad=True)")
        inputs = inputs.reshape(-1, C, H, W)
        _, outputs_vlad = _unwrap(self.model).forward_train(inputs, train_layers=_train_layers(self.model))
        return self._get_loss(outputs_vlad, loss_type, B, N)

    def _get_loss(self, outputs, loss_type, B, N):
        """outputs [B*N][L], tuple-major (anchor, positive, N - 2 negatives) -> the loss: 'triplet' with the trainer's
        margin, 'sare_joint' / 'sare_ind' on the score -|a - x|^2 (the reference's "original version")."""
        _check_loss_type(loss_type)
        outputs = outputs.view(B, N, -1)
        return ops.tuple_loss(outputs[:, 0], outputs[:, 1], outputs[:, 2:], loss_type, margin=self.margin,
                              temp=self.temp, score="sqdist")


class SFRSTrainer(object):
    """Training module for "Self-supervising Fine-grained Region Similarities for Large-scale Image Localization".
    `model` (the student) and `model_cache` (the frozen previous generation) are EmbedRegionNets whose tuple_size is
    the number of tuples per batch."""

    def __init__(self, model, model_cache, margin=0.3,
                 neg_num=10, gpu=None, temp=[0.07, ], augment=None, prefetch=False):
        super(SFRSTrainer, self).__init__()
        self.model = model
        self.model_cache = model_cache
        self.augment = augment      # as Trainer.augment
        self.prefetch = prefetch    # as Trainer.prefetch
        self._files = collections.deque()

        self.margin = margin
        self.gpu = gpu
        self.neg_num = neg_num
        self.temp = temp

    def train(self, gen, epoch, sub_id, data_loader, optimizer, train_iters,
              print_freq=1, lambda_soft=0.5, loss_type='sare_ind'):
        _check_loss_type(loss_type)
        self.model.train()
        self.model_cache.train()

        batch_time, data_time = AverageMeter(), AverageMeter()
        losses_hard, losses_soft = AverageMeter(), AverageMeter()
        end = time.time()
        data_loader.new_epoch()

        self._files.clear()
        ahead = _Prefetch(self._parse_data, data_loader, train_iters, self.gpu) if self.prefetch else None
        for i in range(train_iters):
            inputs_easy, inputs_diff = ahead.take() if ahead else self._parse_data(data_loader.next())
            data_time.update(time.time() - end)

            loss_hard, loss_soft = self._forward(inputs_easy, inputs_diff, loss_type, gen)
            loss = loss_hard + loss_soft * lambda_soft

            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            if ahead:
                ahead.issue()

            losses_hard.update(loss_hard.item())
            losses_soft.update(loss_soft.item())
            _check_files(self._files)

            batch_time.update(time.time() - end)
            end = time.time()

            if (i + 1) % print_freq == 0 and _rank() == 0:
                print('Epoch: [{}-{}][{}/{}]\t'
                      'Time {:.3f} ({:.3f})\t'
                      'Data {:.3f} ({:.3f})\t'
                      'Loss_hard {:.3f} ({:.3f})\t'
                      'Loss_soft {:.3f} ({:.3f})'
                      .format(epoch, sub_id, i + 1, train_iters,
                              batch_time.val, batch_time.avg,
                              data_time.val, data_time.avg,
                              losses_hard.val, losses_hard.avg,
                              losses_soft.val, losses_soft.avg))

    def _parse_data(self, inputs):
        if _is_file_tuples(inputs):
            # the files' bytes: decoded, jittered (every image once, as below) and resized on the device
            imgs = _decode_tuples(self.augment, inputs, self.gpu, self._files)
        else:
            imgs = self._parse_tensors(inputs)
        # easy: anchor, positive, neg_num negatives; diff: anchor and the difficult positives behind them
        imgs_easy = imgs[:, :self.neg_num + 2]
        imgs_diff = torch.cat((imgs[:, :1], imgs[:, self.neg_num + 2:]), dim=1)
        return imgs_easy.cuda(self.gpu), imgs_diff.cuda(self.gpu)

    def _parse_tensors(self, inputs):
        imgs = _stack_tuples(inputs)
        if self.augment is not None:
            # every image is jittered once, the anchor included: the easy and the difficult part share the anchor's
            # jittered image, and the teacher and the student see the same inputs_diff, as in the reference
            imgs = _augment_tuples(self.augment, imgs, self.gpu)
        return imgs

    def _forward(self, inputs_easy, inputs_diff, loss_type, gen):
        _check_loss_type(loss_type)
        B, _, C, H, W = inputs_easy.size()
        inputs_easy = inputs_easy.reshape(-1, C, H, W)
        inputs_diff = inputs_diff.reshape(-1, C, H, W)
        model, layers = _unwrap(self.model), _train_layers(self.model)

        # sim_easy [B][1 + neg_num][9][9], vlad_anchors [B][1][9][L], vlad_pairs [B][1 + neg_num][9][L]
        sim_easy, vlad_anchors, vlad_pairs = model.forward_train(inputs_easy, train_layers=layers)
        with torch.no_grad():
            sim_diff_label, _, _ = _unwrap(self.model_cache).region_similarity(inputs_diff)
        sim_diff, _, _ = model.forward_train(inputs_diff, train_layers=layers)

        anchors, positives = vlad_anchors[:, 0, 0], vlad_pairs[:, 0, 0]
        if gen == 0:
            loss_hard = self._get_loss(anchors, positives, vlad_pairs[:, 1:, 0], B, loss_type)
        else:
            loss_hard = self._get_hard_loss(anchors, positives, vlad_pairs[:, 1:], sim_easy[:, 1:, 0].detach(),
                                            loss_type)

        loss_soft = ops.soft_label_loss(sim_diff[:, :, 0].reshape(B, -1), sim_diff_label[:, :, 0].reshape(B, -1),
                                        self.temp[0], self.temp[gen])
        return loss_hard, loss_soft

    def hard_regions(self, score_neg):
        """score_neg [B][neg_num][9] (or [neg_num][9]), detached: the region of every negative that is most similar
        to the anchor's whole image — argmax over the 9 regions."""
        return score_neg.detach().argmax(-1)

    def _get_hard_loss(self, anchors, positives, negatives, score_neg, loss_type):
        """The hard loss from generation 1 on, for the WHOLE batch: anchors [B][L], positives [B][L], negatives
        [B][neg_num][9][L] (all nine regions), score_neg [B][neg_num][9] = sim_easy[:, 1:, 0] detached.  For every
        negative the region with the highest score is selected — one argmax and one gather — and one fused tuple loss
        runs on the result.  The reference calls its `_get_hard_loss` once per tuple (with B = 1) and averages:
        loss_hard = (1 / B) sum_t loss(tuple t).  Every loss here is a mean over the tuples of per-tuple means with the
        same number of terms per tuple, so the one call over the batch is mathematically that per-tuple sum divided
        by B.  A single tuple ([L], [L], [neg_num][9][L], [neg_num][9]), the reference's signature, is accepted too."""
        _check_loss_type(loss_type)
        if anchors.dim() == 1:
            anchors, positives, negatives, score_neg = anchors[None], positives[None], negatives[None], score_neg[None]
        B, n, R, L = negatives.shape
        arg = self.hard_regions(score_neg.reshape(B, n, R))
        select = torch.gather(negatives, 2, arg.view(B, n, 1, 1).expand(B, n, 1, L))[:, :, 0]
        return self._get_loss(anchors, positives, select, B, loss_type)

    def _get_loss(self, output_anchors, output_positives, output_negatives, B, loss_type):
        """anchors [B][L], positives [B][L], negatives [B][neg_num][L] (views welcome) -> the loss: 'triplet' with the
        trainer's margin, 'sare_joint' / 'sare_ind' on the score <a, x> / temp[0]."""
        _check_loss_type(loss_type)
        return ops.tuple_loss(output_anchors, output_positives, output_negatives, loss_type, margin=self.margin,
                              temp=self.temp[0], score="dot")
