"""The fail-safe protocol of the chained launches (tg_srnet_body_fwd / _bwd, csrc/tg_conv3x3_chain.hip): the process-wide
state of those launches (flag buffers, epoch counter, pinned fault counter, fallback switch and its re-arm), the stamp that
carries a fault into the optimiser's guarded step, and the check that raises it once.  The tape node that issues the
launches is models/train_graph.py: srnet_body."""
import torch

from .. import ops


class _ChainState:
    """Process-wide state of the chained launches: flag buffers per shape, the epoch counter, the
    pinned-host fault counter (the kernel adds to it with system scope when a workgroup gives up
    waiting for a neighbour) and the permanent fallback switch."""
    disabled = False
    poll_limit = 1 << 21
    epoch = 0
    flags = {}
    err = None
    supported = {}
    dirty = False           # chained launches were enqueued since the last SYNCHRONOUS look at the counter
    reported_epoch = 0      # launches up to this epoch are covered by a fault that has already been raised
    # Recovery from a transient fault (round 6, as in the frame plan: tg_frnet_plan_set_chain_rearm): after `rearm_wait`
    # clean ITERATIONS on the per-layer path (counted by chain_check, which every rank calls once per iteration, and a
    # fault reaches every rank through the all-reduced slot: the count is rank-symmetric) the chained body launches are
    # tried again; a fault of the re-armed launches doubles the wait.  rearm_first = 0: off for good (rounds 3-5).
    rearm_first = 64
    rearm_wait = 0
    clean_iters = 0
    rearms = 0

    @classmethod
    def note_fault(cls):
        cls.disabled = True
        cls.clean_iters = 0
        cls.rearm_wait = min(2 * cls.rearm_wait, 1 << 20) if cls.rearm_wait else cls.rearm_first

    @classmethod
    def note_clean_iteration(cls):
        if cls.disabled and cls.rearm_first > 0 and cls.rearm_wait > 0:
            cls.clean_iters += 1
            if cls.clean_iters >= cls.rearm_wait:
                cls.disabled = False
                cls.clean_iters = 0
                cls.rearms += 1

    @classmethod
    def buffers(cls, nlayer, n, h, w, device):
        from .. import _lib as L
        # one flag buffer per (shape, device, stream): two chained launches of one shape in flight at once
        # (a second model, a side stream, another device) must not overwrite each other's epochs
        key = (n, h, w, str(device), ops._stream())
        fl = cls.flags.get(key)
        need = L.lib().tg_conv3x3_chain_flag_ints(24, n, h, w)
        if fl is None or fl.numel() < need:
            fl = cls.flags[key] = torch.zeros(need, dtype=torch.int32, device=device)
        if cls.err is None:
            cls.err = torch.zeros(16, dtype=torch.int32).pin_memory()
        cls.epoch = cls.epoch + 1 if cls.epoch < 0x7fffffff else 1
        cls.dirty = True
        return fl, cls.err, cls.epoch

    @classmethod
    def parts(cls, n, h, w):
        """workgroups per tile the launcher uses for this shape (0: not supported): 4 needs the
        16 x 16 x 4 weight layout (ops.pack_conv3x3_m16), 1 / 2 the 64-channel-block layout."""
        key = (n, h, w, torch.cuda.current_device() if torch.cuda.is_available() else -1)
        r = cls.supported.get(key)
        if r is None:
            from .. import _lib as L
            r = cls.supported[key] = int(L.lib().tg_conv3x3_chain_supported(n, h, w, 64))
        return r

    MAX_LAYERS = 24      # RC_MAXL of tg_conv3x3_chain.hip: tg_srnet_body_fwd / _bwd walk 1 + 2 nb (+ 1) layers

    @classmethod
    def usable(cls, n, nf, cin0, h, w, nb):
        """nb: residual blocks of the body (a free yml parameter in the reference, tecogan_nets.py:108-116):
        beyond 11 the body does not fit one chained launch and runs one launch per layer."""
        if cls.disabled or nf > 64 or cin0 > 64 or nb < 1 or 2 * nb + 2 > cls.MAX_LAYERS:
            return False
        return cls.parts(n, h, w) > 0


def _distributed_world():
    """Ranks of the initialised process group; 1 without one."""
    try:
        import torch.distributed as dist
        return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    except ImportError:
        return 1


def guard_available(optim):
    """The device-side guard of the chained launches' fail-safe exists for this optimiser: its flat gradient buffer
    (with the fault slot behind the last tensor) is still what the parameters' .grad views point into."""
    return optim is not None and getattr(optim, 'fault_slot', None) is not None and optim._is_flat()


def stamp_fault(optim):
    """Before a network's gradient exchange / optimiser step: add 1 to the FAULT SLOT of its flat gradient
    buffer if a chained launch of this process has recorded a fault (a one-thread kernel reads the pinned
    counter).  The slot is all-reduced with the gradients and guards the Adam step on the device
    (tg_adam_step_guarded): gradients built on stale tiles are then applied on NO rank.

    An optimiser WITHOUT that slot (`Adam(flatten=False)`, views replaced by `net.to()` / `p.grad = None`) has no
    asynchronous guard: the step then falls back to the synchronous protocol ONCE -- wait for the device, look at the
    counter (on every rank: one max-all-reduce of the flag), raise BEFORE the update is applied -- and every later
    step runs one launch per layer, so the check is never needed again."""
    err = _ChainState.err
    if err is None or optim is None:
        return
    if guard_available(optim):
        ops.fault_to_slot(err, optim.fault_slot)
        return
    # An optimiser that HAD its flat buffer at construction (every rank compared that: BaseModel.agreement_vector) and
    # lost it on this rank only -- `p.grad = None`, a `net.to()` -- would enter the synchronous protocol below, whose
    # max-all-reduce the other ranks never join: a hang.  A loud rank-local error instead (the peers then fail in RCCL's
    # own time-out rather than waiting for ever).
    if getattr(optim, 'fault_slot', None) is not None and _distributed_world() > 1:
        from .. import _lib as L_
        raise L_.TecoganHipError(
            'an optimiser of a data-parallel run lost its flat gradient buffer on this rank (the .grad views were '
            'replaced): the device-side fault guard and the one-collective gradient exchange are rank-symmetric by '
            'construction -- rebuild the optimiser on every rank (Adam(..., flatten=True)) instead')
    if not _ChainState.dirty:
        return
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _ChainState.dirty = False
    _ChainState.disabled = True          # (for good: without the device-side guard every chained step would need this sync)
    _ChainState.rearm_wait = 0
    local = int(err[0]) != 0
    anywhere = local
    if _distributed_world() > 1:
        from ..utils import dist_utils
        anywhere = dist_utils.max_over_ranks(1.0 if local else 0.0, device=optim.params[0].device) != 0.0
    if anywhere:
        chain_check(0.0 if local else 1.0, counter=True)


def chain_check(slot_value=0.0, counter=True, epoch=None):
    """Raises if a chained launch recorded a fault: on any rank in the iteration whose scalars are being looked at
    (`slot_value`: the fault slot of the generator's gradient buffer after its all-reduce, read with that iteration's
    scalars), or -- `counter`, for callers that have just synchronised the device -- on this rank since the last check
    (pinned counter).  The training step resolves its scalars asynchronously (base_model: a later iteration may
    already be in flight and adding to the counter), so it passes counter=False and relies on the slot, which is
    exact per iteration; the counter is cleared only after a device synchronisation.  The iteration's generator
    update was dropped on every rank by the device-side guard; every later step runs one launch per layer.

    `epoch`: the chained-launch epoch at which the iteration was stamped.  An iteration that was already in flight
    when an earlier one raised carries the same fault in its slot (the pinned counter is cleared only by the raise):
    it is reported ONCE -- the call then returns True (update dropped, nothing raised).  Returns False when the
    iteration is clean."""
    err = _ChainState.err
    local = counter and err is not None and int(err[0]) != 0
    if not (local or slot_value != 0.0):
        if not counter:                  # (the per-iteration call of the training step)
            _ChainState.note_clean_iteration()
        return False
    if not local and epoch is not None and epoch <= _ChainState.reported_epoch:
        return True
    from .. import _lib as L
    if torch.cuda.is_available():
        torch.cuda.synchronize()            # nothing in flight may add to the counter after it is cleared
    lost = int(err[0]) if err is not None else 0
    if err is not None:
        err.zero_()
    _ChainState.note_fault()
    _ChainState.dirty = False
    _ChainState.reported_epoch = _ChainState.epoch     # everything enqueued so far has completed (synchronised above)
    raise L.TecoganHipError(
        'chained SRNet launch (training): %s timed out waiting for a neighbour tile; the results of this '
        'step are INVALID and its optimiser step was DROPPED on every rank (weights and Adam moments '
        'untouched).  Later steps run one launch per layer%s.'
        % (f'{lost} workgroup(s) of this rank' if lost else 'workgroups of another rank',
           f'; the chained launches are tried again after {_ChainState.rearm_wait} clean iterations'
           if _ChainState.rearm_first > 0 else ''))


def chain_epoch():
    """The epoch of the last chained launch enqueued by this process (see chain_check)."""
    return _ChainState.epoch
