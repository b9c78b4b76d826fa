"""VSRModel (FRVSR): generator only, Charbonnier pixel + warping loss
(codes/models/vsr_model.py)."""
from collections import OrderedDict

import torch

from .. import ops
from . import train_chain
from . import train_graph as TG
from .base_model import BaseModel, front_pad_stream
from .networks import define_generator
from .optim import Adam, define_criterion, define_lr_schedule, pointwise_loss


class VSRModel(BaseModel):
    def __init__(self, opt):
        super().__init__(opt)
        self.set_networks()
        if self.is_train:
            self.set_criterions()
            self.set_optimizers()
            self.check_ranks_agree()

    def set_networks(self):
        self.net_G = self.model_to_device(define_generator(self.opt))
        load_path_G = self.opt['model']['generator'].get('load_path')
        if load_path_G:
            self.load_network(self.net_G, load_path_G)

    def set_criterions(self):
        self.pix_crit = define_criterion(self.opt['train'].get('pixel_crit'))
        self.warp_crit = define_criterion(self.opt['train'].get('warping_crit'))

    def set_optimizers(self):
        g = self.opt['train']['generator']
        self.optim_G = Adam(self.net_G.parameters(), lr=g['lr'],
                            weight_decay=g.get('weight_decay', 0), betas=g.get('betas', (0.9, 0.999)))
        self.sched_G = define_lr_schedule(g.get('lr_schedule'), self.optim_G)

    # -- loss helpers (value accumulates on the device; gradient returned) -----
    @staticmethod
    def _crit(crit, x, y, weight, acc):
        return pointwise_loss(crit, x, y, weight, acc)

    def train(self):
        """vsr_model.py:61-95."""
        self.net_G.train()
        self.optim_G.zero_grad()
        out = self.net_G(self.lr_data)
        tape = self.net_G.tape
        self.hr_data = out['hr_data']
        losses = torch.zeros(3, dtype=torch.float32, device=self.device)     # [pixel, warp, fault slot]
        pix_w = self.opt['train']['pixel_crit'].get('weight', 1.0)
        tape.add_grad(out['hr_data'], self._crit(self.pix_crit, out['hr_data'],
                                                 self.gt_data.contiguous(), pix_w, losses[0:1]))
        if self.warp_crit is not None:
            lr_warp = TG.backward_warp(tape, out['lr_prev'], out['lr_flow'], need_dimg=False)
            warp_w = self.opt['train']['warping_crit'].get('weight', 1.0)
            tape.add_grad(lr_warp, self._crit(self.warp_crit, lr_warp, out['lr_curr'], warp_w,
                                              losses[1:2]))
        tape.backward()
        train_chain.stamp_fault(self.optim_G)                 # a chained-launch fault (any rank) turns the step into a no-op
        self.allreduce_grads(self.net_G, 'G')
        self.optim_G.step()
        if getattr(self.optim_G, 'fault_slot', None) is not None:
            losses[2:3].copy_(self.optim_G.fault_slot)
        has_warp = self.warp_crit is not None
        ep, optim_G = train_chain.chain_epoch(), self.optim_G

        def build(vals):                             # runs when the log is looked at (base_model: asynchronous scalars)
            try:                                     # fail-safe of the chained launches: raises on EVERY rank, the update was dropped
                dropped = train_chain.chain_check(vals[2], counter=False, epoch=ep)
            except Exception:
                optim_G.undo_step_count()
                raise
            if dropped:                              # in flight behind an iteration that already raised
                optim_G.undo_step_count()
            d = OrderedDict(l_pix_G=vals[0])
            if has_warp:
                d['l_warp_G'] = vals[1]
            return d
        self._set_pending_log(losses, build)

    def infer(self, device_output=False):
        """vsr_model.py:97-113: temporal padding, inference, crop the padding back.
        device_output=True keeps the (t,H,W,3) uint8 result on the GPU (for the on-device
        PSNR) instead of returning the reference's numpy array."""
        lr_data, n_pad_front = self.pad_sequence(self.lr_data)
        self.net_G.eval()
        if device_output:
            hr_seq = self.net_G.infer_sequence(lr_data, self.device, return_device_tensor=True)
        else:
            hr_seq = self.net_G(lr_data, self.device)
        return hr_seq[n_pad_front:]

    def infer_stream(self, frames, yuv=None, scene_cut=None, png=None, resize=None, deinterlace=None):
        """infer() for a clip of any length (FRNet.infer_stream): `frames` is an iterable of LR frames or chunks, uint8
        (h,w,3) or float32 (3,h,w); yields (m,H,W,3) uint8 chunks -- views of the generator's pinned ring, valid until
        the next one is asked for.  The temporal padding of the front (test.padding_mode / num_pad_front) is applied
        lazily: the first n_pad + 1 frames are buffered, the padded prefix runs first, its n_pad outputs are dropped.
        yuv (a Yuv420, or a Yuv for 4:2:2 / 4:4:4 / BT.2020): the items are planar YUV frames or chunks of them and
        (m, out_frame_bytes) chunks of such frames are yielded.
        png (a Png): lists of 1-D uint8 views are yielded, each view one complete PNG file (not together with yuv);
        Png(lz77=True) makes them smaller and the stream slower.
        scene_cut (a SceneCut): the recurrence restarts at scene cuts (FRNet.infer_stream).  Its `at`, `cuts` and
        `scores` are in the numbering of `frames`: the padded stream runs a shifted copy, and what that finds inside
        the padded prefix is dropped.  Known limit: the front padding is NOT repeated after a cut -- a new shot starts
        cold, as a clip does with num_pad_front = 0.
        resize (a Resize): every frame is delivered at resize.h x resize.w, resized on the device, in whichever of the
        three output forms (FRNet.infer_stream).
        deinterlace (a Deinterlace, with yuv): the items are INTERLACED frames and two progressive frames per item are
        yielded (one at rate 'frame'), deinterlaced on the device (FRNet.infer_stream).  Interlaced
        frames reflected in time are not a sequence of real fields, so with deinterlace the FRONT PADDING IS SKIPPED
        whatever test.num_pad_front says: the stream starts cold, as FRNet.infer_stream does, one log line says so, and
        scene_cut behaves as scene_cut.shifted(0) -- its indices are output frames."""
        mode = self.opt['test'].get('padding_mode', 'reflect')
        skip = self.opt['test'].get('num_pad_front', 0)
        if deinterlace is not None and skip:
            import logging
            logging.getLogger('tecogan_pytorch_amd').info(
                'infer_stream: deinterlace: the front padding (num_pad_front = %d) is skipped, the stream starts cold', skip)
            skip = 0
        self.net_G.eval()
        n_pad, inner, seen = skip, None, (0, 0)
        if scene_cut is not None:
            inner = scene_cut.shifted(n_pad)
            scene_cut.cuts.clear()
            scene_cut.scores.clear()
        gen = self.net_G.infer_stream(front_pad_stream(frames, mode, skip, self.net_G.in_nc, yuv), self.device,
                                      yuv=yuv, **({} if inner is None else {'scene_cut': inner}),
                                      **({} if png is None else {'png': png}),
                                      **({} if resize is None else {'resize': resize}),
                                      **({} if deinterlace is None else {'deinterlace': deinterlace}))
        try:
            for chunk in gen:
                if inner is not None:
                    seen = scene_cut.absorb(inner, n_pad, seen)
                if skip >= len(chunk):
                    skip -= len(chunk)
                    continue
                yield chunk[skip:]
                skip = 0
        finally:
            gen.close()

    def save(self, current_iter):
        self.sync_log()          # (a pending fault check must run before weights are written)
        self.save_network(self.net_G, 'G', current_iter)
