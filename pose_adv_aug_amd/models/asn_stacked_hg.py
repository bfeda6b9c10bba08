"""models/asn_stacked_hg.py of the reference behind the HIP engine.

`create_hg` / `create_asn` keep the reference's signatures (models/asn_stacked_hg.py:344-347, :441-444)
and return objects with the nn.Module surface the reference's scripts use -- __call__/forward,
state_dict / load_state_dict (same names, NCHW shapes and order as the reference's modules),
parameters(), train(), eval(), cuda() -- but the arithmetic runs in libposeadv_hip.so on flat fp32
parameter / gradient buffers; torch only owns the memory.  There is no autograd graph: use
`loss_and_backward()` (the fused forward + loss + hand-written backward) instead of loss.backward().
"""
import ctypes as C
import math
from collections import OrderedDict

import numpy as np
import torch

from .. import _lib
from .._lib import lib, check, ptr, stream, require_gpu, PoseAdvError


class _HipModule(object):
    """Flat-buffer module: parameters / gradients / running statistics live in three flat fp32 GPU
    tensors laid out by the C library (pa_net_tensor_info), state_dict entries are views into them."""

    def __init__(self):
        self.training = True
        self._nets = {}          # batch size -> (handle, workspace tensor)
        self._table = None
        self.flat_params = self.flat_grads = self.flat_buffers = None
        self._nbt = 0            # num_batches_tracked (identical for every BatchNorm of the module)
        self._weights_dirty = True

    # -- to be provided by subclasses
    def _create(self, B):
        raise NotImplementedError

    # -- handle management
    def _read_table(self, h):
        L = lib()
        table = []
        name = C.create_string_buffer(256)
        shape = (C.c_int * 4)(); nd = C.c_int(); off = C.c_size_t(); numel = C.c_size_t(); kind = C.c_int()
        for i in range(L.pa_net_num_tensors(h)):
            check(L.pa_net_tensor_info(h, i, name, 256, shape, C.byref(nd), C.byref(off), C.byref(numel), C.byref(kind)))
            table.append((name.value.decode(), tuple(shape[k] for k in range(nd.value)), off.value, numel.value, kind.value))
        return table

    def _net(self, B):
        require_gpu()
        if B not in self._nets:
            L = lib()
            h = self._create(B)
            if not h:
                raise PoseAdvError('network creation failed: %s' % L.pa_last_error().decode())
            dev = _lib.device()
            if self._table is None:
                self._table = self._read_table(h)
                self.flat_params = torch.zeros(L.pa_net_param_floats(h), dtype=torch.float32, device=dev)
                self.flat_grads = torch.zeros_like(self.flat_params)
                self.flat_buffers = torch.zeros(max(1, L.pa_net_buffer_floats(h)), dtype=torch.float32, device=dev)
                for name, shape, off, numel, kind in self._table:
                    if kind == 1 and name.endswith('running_var'):
                        self.flat_buffers[off:off + numel] = 1.0
                self.reset_parameters()
            ws = torch.empty(L.pa_net_workspace_bytes(h), dtype=torch.uint8, device=dev)       # (pa_net_bind clears it)
            check(L.pa_net_bind(h, ptr(self.flat_params), ptr(self.flat_grads), ptr(self.flat_buffers), ptr(ws), stream()),
                  'pa_net_bind')
            self._nets[B] = (h, ws)               # (binding packs THIS handle's bf16 weights; a pending change still has to reach
            if len(self._nets) == 1:              #  the handles of the other batch sizes, so the flag survives unless this is the only one)
                self._weights_dirty = False
        h, _ = self._nets[B]
        if self._weights_dirty:
            for hh, _ in self._nets.values():
                check(lib().pa_net_prepare_weights(hh), 'pa_net_prepare_weights')
            self._weights_dirty = False
        return h

    def _ensure_table(self):
        if self._table is None:
            self._net(self.default_batch)

    def __del__(self):
        try:
            for h, _ in self._nets.values():
                lib().pa_net_destroy(h)
        except Exception:
            pass

    # -- nn.Module surface
    def weights_changed(self):
        """Call after writing into parameter views (optimizer step, load_state_dict)."""
        self._weights_dirty = True

    def named_parameters(self):
        self._ensure_table()
        for name, shape, off, numel, kind in self._table:
            if kind == 0:
                yield name, self.flat_params[off:off + numel].view(shape)

    def parameters(self):
        return [p for _, p in self.named_parameters()]

    def named_grads(self):
        """views into flat_grads; they carry _lib.grad_scale() (1 for the bf16 build)"""
        self._ensure_table()
        for name, shape, off, numel, kind in self._table:
            if kind == 0:
                yield name, self.flat_grads[off:off + numel].view(shape)

    def state_dict(self, prefix=''):
        self._ensure_table()
        sd = OrderedDict()
        for name, shape, off, numel, kind in self._table:
            if kind == 0:
                sd[prefix + name] = self.flat_params[off:off + numel].view(shape)
            elif kind == 1:
                sd[prefix + name] = self.flat_buffers[off:off + numel].view(shape)
            else:
                sd[prefix + name] = torch.tensor(self._nbt, dtype=torch.long)
        return sd

    def load_state_dict(self, state_dict, strict=True):
        own = self.state_dict()
        missing = [k for k in own if k not in state_dict and 'module.' + k not in state_dict]
        unexpected = []
        for k, v in state_dict.items():
            kk = k[7:] if k.startswith('module.') else k        # reference checkpoints carry DataParallel's prefix
            if kk not in own:
                unexpected.append(k)
                continue
            if kk.endswith('num_batches_tracked'):
                self._nbt = int(v)
                continue
            own[kk].copy_(torch.as_tensor(v).to(own[kk].device, torch.float32).view_as(own[kk]))
        if strict and (missing or unexpected):
            raise KeyError('load_state_dict: missing %s unexpected %s' % (missing[:5], unexpected[:5]))
        self.weights_changed()
        return missing, unexpected

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def cuda(self, *a, **k):
        require_gpu()
        return self

    def zero_grad(self):
        if self.flat_grads is not None:
            self.flat_grads.zero_()

    def num_params(self):
        return sum(n for _, _, _, n, k in (self._table or []) if k == 0)

    def reset_parameters(self, seed=None):
        """The reference's initialisation (models/asn_stacked_hg.py:258-270): conv weight and bias
        U(+-1/sqrt(k*k*Cin)), BatchNorm gamma U(0,1), beta 0; Linear layers keep torch's default."""
        if self._table is None:
            self._net(self.default_batch)          # creates the buffers and calls back into this method
            if seed is None:
                return
        g = torch.Generator().manual_seed(int(seed) if seed is not None else torch.initial_seed() % (2 ** 31))
        bound = None
        for name, shape, off, numel, kind in self._table:
            if kind != 0:
                continue
            if len(shape) == 4:
                bound = 1.0 / math.sqrt(shape[1] * shape[2] * shape[3])
                v = (torch.rand(shape, generator=g) * 2 - 1) * bound
            elif len(shape) == 2:                               # nn.Linear default: U(+-1/sqrt(fan_in))
                bound = 1.0 / math.sqrt(shape[1])
                v = (torch.rand(shape, generator=g) * 2 - 1) * bound
            elif _is_bn_name(name):
                v = torch.rand(shape, generator=g) if name.endswith('weight') else torch.zeros(shape)
            else:                                               # bias of the conv / linear just declared
                v = (torch.rand(shape, generator=g) * 2 - 1) * bound
            self.flat_params[off:off + numel] = v.reshape(-1).to(self.flat_params.device)
        self.weights_changed()


def _is_bn_name(name):
    leaf = name.rsplit('.', 2)
    mod = leaf[-2] if len(leaf) >= 2 else ''
    if mod.startswith('bn'):
        return True
    return mod == '1' and '.linear.' in '.' + name        # linear.<i>.1 is the BatchNorm of the Sequential


class _HeatMapsFunction(torch.autograd.Function):
    """HourglassNet.forward_autograd: the engine's forward pass as ONE autograd node with num_stacks outputs.  `anchor` is the module's
    private one-element leaf (requires_grad): it makes the outputs part of a graph; it gets no gradient -- the parameter gradients go
    to net.flat_grads through HourglassNet.backward()."""

    @staticmethod
    def forward(ctx, anchor, net, x, img4, pts, dropout_masks, layout):
        outs = net._forward(x, img4, pts, dropout_masks, layout)
        ctx.net, ctx.serial, ctx.done, ctx.layout = net, net._fwd_serial, False, layout
        # which input carries the image: its gradient (HourglassNet.backward(input_grad=...)) is returned when autograd asks for it
        ctx.img4_dtype = img4.dtype if img4 is not None else None      # (the engine reads img4 when it is given)
        ctx.set_materialize_grads(False)                # a stack the loss does not use arrives as None = zero, not as a tensor of zeros
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        net = ctx.net
        if ctx.done:
            raise RuntimeError('forward_autograd: backward ran a second time for the same forward pass (the engine keeps no graph to retain)')
        if net._fwd_serial != ctx.serial:
            raise RuntimeError('forward_autograd: another forward pass of this net has run since these heat maps were made; '
                               'its stored activations are gone')
        ctx.done = True
        want_x, want_img4 = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if want_x and ctx.img4_dtype is None:
            return (None, None, net.backward(grads, ctx.layout, input_grad='nchw'), None, None, None, None)
        if want_img4 and ctx.img4_dtype is not None:
            return (None, None, None, net.backward(grads, ctx.layout, input_grad='nhwc4').to(ctx.img4_dtype), None, None, None)
        net.backward(grads, ctx.layout)
        return (None,) * 7


class HourglassNet(_HipModule):
    """_Hourglass_Wrapper of the reference (models/asn_stacked_hg.py:215-342)."""

    def __init__(self, num_modules, num_stacks, chan=256, num_classes=16, res=256, default_batch=24):
        super().__init__()
        if int(num_modules) != num_modules or not 1 <= num_modules <= 8:
            raise ValueError('num_modules must be an integer from 1 to 8 (residual blocks per site), got %r' % (num_modules,))
        self.num_modules = int(num_modules)
        self.num_stacks, self.chan, self.num_classes, self.res = num_stacks, chan, num_classes, res
        self.default_batch = default_batch
        self._last_B = None

    def _twin(self):
        """a new net of the same configuration with its own flat arrays and handles (utils.optim.ModelEma)"""
        return HourglassNet(self.num_modules, self.num_stacks, chan=self.chan, num_classes=self.num_classes, res=self.res,
                            default_batch=self.default_batch)

    def _create(self, B):
        if self.num_modules == 1:
            return lib().pa_hg_create(self.num_stacks, self.num_classes, self.chan, B, self.res)
        return lib().pa_hg_create_modules(self.num_stacks, self.num_modules, self.num_classes, self.chan, B, self.res)

    def forward(self, x=None, asn=None, is_half_hg=False, is_aug=False, is_dropout=False, img4=None, pts=None,
                dropout_masks=None, seed=0):
        """models/asn_stacked_hg.py:282-342.  x: [B][3][res][res] fp32 GPU tensor (or img4: the bf16
        NHWC4 output of the on-device warp).  Returns the list of per-stack heat maps [B][16][res/4][res/4]
        (fp32, NCHW) like the reference.  With `asn` and is_half_hg the agent's two logit tensors.
        Occlusion branch (:308-324): with an is_dropout agent, is_half_hg gives the [B][1][4][4] mask logits; the whole
        hourglass draws two cells per sample from their softmax on the device (stream: `seed` and a per-module call
        counter), zeroes them in the neck / skip tensors of every stack and returns (outs, pred_mask, indexes); the
        drawn masks stay in `last_dropout_masks` for loss_and_backward(dropout_masks=...).  `dropout_masks`
        ([B][1][4][4], without an agent) applies given masks (:183-189)."""
        if asn is not None:
            assert is_aug != is_dropout                      # :299
            if is_aug:
                return asn._forward_from_pose(self, x, img4, is_half_hg)
            assert dropout_masks is None                     # :160
            pred_mask = asn._forward_masks_from_pose(self, x, img4, update_running=is_half_hg)
            if is_half_hg:
                return pred_mask
            masks, indexes = sample_mask(pred_mask, seed=seed, step=self._drop_calls)
            self._drop_calls += 1
            self.last_dropout_masks = masks
            return self._forward(x, img4, pts, masks), pred_mask, indexes
        return self._forward(x, img4, pts, dropout_masks)

    __call__ = forward
    _drop_calls = 0
    last_dropout_masks = None

    def _set_masks(self, h, masks):
        """pa_hg_set_dropout_masks with a [B][1][4][4] (or [B][16]) mask tensor, None = off; returns the tensor to keep alive"""
        if masks is None:
            check(lib().pa_hg_set_dropout_masks(h, None), 'pa_hg_set_dropout_masks')
            return None
        m = masks.to(self.flat_params.device, torch.float32).reshape(masks.shape[0], 16).contiguous()
        check(lib().pa_hg_set_dropout_masks(h, ptr(m)), 'pa_hg_set_dropout_masks')
        return m

    _last_masks = None       # the dropout masks of the last forward pass (backward() sets them again around its pass)
    _fwd_serial = 0          # counts the forward passes (whole or half) of this net: forward_autograd's backward needs ITS pass's activations

    def _forward(self, x, img4, pts, dropout_masks=None, layout='nchw'):
        if layout not in ('nchw', 'nhwc'):
            raise ValueError("layout must be 'nchw' or 'nhwc', got %r" % (layout,))
        B = x.shape[0] if x is not None else img4.shape[0]
        h = self._net(B)
        self._last_B = B
        self._fwd_serial += 1
        self._last_masks = dropout_masks
        p = pts.to(torch.float64).contiguous() if pts is not None else None
        losses = torch.empty(self.num_stacks, dtype=torch.float32, device=self.flat_params.device) if pts is not None else None   # (fully overwritten)
        keep = self._set_masks(h, dropout_masks)
        try:
            check(lib().pa_hg_forward(h, ptr(x.contiguous().float()) if x is not None else None, ptr(img4), ptr(p),
                                      1 if self.training else 0, ptr(losses)), 'pa_hg_forward')
        finally:
            if keep is not None:                             # (stream-ordered: `keep` outlives the kernels that read it)
                self._set_masks(h, None)
        if self.training:
            self._nbt += 1
        self._last_losses = losses
        return self.heatmaps(B, layout)

    def heatmaps(self, B=None, layout='nchw'):
        """The per-stack heat maps of the last forward pass at batch size B.  'nchw' (default): new tensors [B][16][res/4][res/4], one
        conversion launch per stack.  'nhwc': [B][res/4][res/4][16] VIEWS of the engine's own buffers (pa_hg_heatmap_nhwc), no launch and
        no copy -- valid until the next forward pass of this net overwrites them (clone what has to outlive it), and not to be written."""
        if layout not in ('nchw', 'nhwc'):
            raise ValueError("layout must be 'nchw' or 'nhwc', got %r" % (layout,))
        B = B or self._last_B
        h = self._net(B)
        outs = []
        if layout == 'nhwc':
            ws, Hh = self._nets[B][1], self.res // 4
            nbytes = B * Hh * Hh * 16 * 4
            for i in range(self.num_stacks):
                off = lib().pa_hg_heatmap_nhwc(h, i) - ws.data_ptr()          # the pointer lies in the workspace tensor this module owns
                if off < 0 or off % 16 or off + nbytes > ws.numel():
                    raise PoseAdvError('heatmaps: the heat maps of stack %d are not inside the bound workspace' % i)
                outs.append(ws[off:off + nbytes].view(torch.float32).view(B, Hh, Hh, 16).detach())
            return outs
        for i in range(self.num_stacks):
            o = torch.empty((B, 16, self.res // 4, self.res // 4), dtype=torch.float32, device=self.flat_params.device)
            check(lib().pa_hg_heatmap_nchw(h, i, ptr(o)), 'pa_hg_heatmap_nchw')
            outs.append(o)
        return outs

    use_graph = False        # loss_and_backward(img4=...) replays a captured HIP graph of forward + backward (pa_hg_train_step)
    on_stack_done = None     # callback(stack index) after the backward pass of a stack is enqueued (utils.optim.RMSprop(overlap=True))

    last_input_grad = None   # loss_and_backward(input_grad=...): d loss / d image of that step (a new tensor per step), else None

    @staticmethod
    def _input_grad_layout(input_grad):
        """input_grad of backward() / loss_and_backward() -> None (off), 0 ('nchw' or True: [B][3][res][res]) or 1 ('nhwc4': [B][res][res][4])"""
        if input_grad is False or input_grad is None:
            return None
        if input_grad is True or input_grad == 'nchw':
            return 0
        if input_grad == 'nhwc4':
            return 1
        raise ValueError("input_grad must be False, True, 'nchw' or 'nhwc4', got %r" % (input_grad,))

    def _open_image_grad(self, h, B, lay):
        """pa_hg_set_image_grad with a new fp32 tensor in layout `lay` (None: nothing happens); returns the tensor"""
        if lay is None:
            return None
        shape = (B, 3, self.res, self.res) if lay == 0 else (B, self.res, self.res, 4)
        g = torch.empty(shape, dtype=torch.float32, device=self.flat_params.device)       # (the engine overwrites every element)
        check(lib().pa_hg_set_image_grad(h, ptr(g), lay), 'pa_hg_set_image_grad')
        return g

    def loss_and_backward(self, x=None, pts=None, img4=None, want_outputs=False, dropout_masks=None, after_forward=None,
                          input_grad=False):
        """One pass of stack-hg.py:153-164 without the optimizer: forward in the current mode, loss
        sum_stacks mean((out - gaussian(pts))^2) with the target generated on the fly from `pts`
        ([B][16][2] heat-map coordinates), backward into flat_grads.  Returns (loss 0-d GPU tensor, outputs).
        The loss tensor is a VIEW of one slot of a ring of 16 device floats the engine writes (pa_hg_set_loss_total: no framework
        reduction between backward and optimizer): it holds this step's loss until the 16th later call of this method overwrites
        it -- consume it (meters, .item(), .clone()) before that; the shipped loops read it in the same iteration.
        dropout_masks ([B][1][4][4]): the occlusion masks of the reference's dropout branch, in every stack.
        after_forward: a callable run between the two passes; its accuracy() / pckh_origin_res() calls (stack-hg.py:176-178 read
        nothing but the forward pass's heat maps) go to the engine's meter stream and run BESIDE the backward pass instead of between
        two steps (pa_net_meters_async); their results are ordered behind this call like everything else.  The value it returns is
        kept in self.after_forward_result.  (Not with use_graph: there the two passes are one launch.)
        input_grad (False / True or 'nchw' / 'nhwc4', as in backward()): the step also leaves d loss / d image in self.last_input_grad
        (unscaled fp32; None without it); with use_graph such a call takes the eager path, as one with dropout_masks does."""
        lay = self._input_grad_layout(input_grad)                  # (ValueError before anything is launched)
        B = x.shape[0] if x is not None else img4.shape[0]
        h = self._net(B)
        self._last_B = B
        self._fwd_serial += 1
        self._last_masks = dropout_masks
        p = pts.to(torch.float64).contiguous()
        losses = torch.empty(self.num_stacks, dtype=torch.float32, device=self.flat_params.device)      # the engine copies every entry
        self._last_losses = losses                                  # per-stack values of this step (the returned loss is their sum)
        self.last_input_grad = None
        if self.use_graph and x is None and dropout_masks is None and lay is None:
            check(lib().pa_hg_train_step(h, ptr(img4), ptr(p), 1 if self.training else 0, 1, ptr(losses)), 'pa_hg_train_step')
            if self.training:
                self._nbt += 1
            return losses.sum(), (self.heatmaps(B) if want_outputs else None)
        keep = self._set_masks(h, dropout_masks)
        # the sum over the stacks comes from the engine (pa_hg_set_loss_total): one of 16 rotating device floats, valid until 16 calls later
        if getattr(self, '_loss_ring', None) is None:
            self._loss_ring, self._loss_slot = torch.zeros(16, dtype=torch.float32, device=self.flat_params.device), 0
        self._loss_slot = (self._loss_slot + 1) % 16
        total = self._loss_ring[self._loss_slot:self._loss_slot + 1]
        check(lib().pa_hg_set_loss_total(h, ptr(total)), 'pa_hg_set_loss_total')
        try:
            check(lib().pa_hg_forward(h, ptr(x.contiguous().float()) if x is not None else None, ptr(img4), ptr(p),
                                      1 if self.training else 0, ptr(losses)), 'pa_hg_forward')
            if self.training:
                self._nbt += 1
            if after_forward is not None:
                self._meter_keep = []                           # buffers the meter stream uses: alive until the backward pass has joined it
                check(lib().pa_net_meters_async(h, 1), 'pa_net_meters_async')
                try:
                    self.after_forward_result = after_forward()
                finally:
                    check(lib().pa_net_meters_async(h, 0), 'pa_net_meters_async')
            self.last_input_grad = self._open_image_grad(h, B, lay)
            self._run_backward(h)
            self._meter_keep = None                            # (the backward pass has enqueued the join: later users of these blocks are ordered behind the meters)
            outs = self.heatmaps(B) if want_outputs else None
        finally:
            lib().pa_hg_set_loss_total(h, None)
            if lay is not None:
                lib().pa_hg_set_image_grad(h, None, 0)
            if keep is not None:
                self._set_masks(h, None)
            if getattr(self, '_meter_keep', None) is not None:
                # after_forward() or the backward call raised: the join was never enqueued.  Wait for the meter stream before its
                # buffers go back to the allocator, and stop collecting (later accuracy() calls would grow the list for ever).
                torch.cuda.synchronize()
                self._meter_keep = None
        return total.view(()), outs

    def _run_backward(self, h):
        if self.on_stack_done is not None:                  # the backward pass in phases: a finished stack's gradients can travel
            for phase in range(self.num_stacks + 1):
                check(lib().pa_hg_backward_phase(h, phase), 'pa_hg_backward_phase')
                if phase < self.num_stacks:
                    self.on_stack_done(self.num_stacks - 1 - phase)
        else:
            check(lib().pa_hg_backward(h), 'pa_hg_backward')

    def backward(self, grad_outputs, layout='nchw', input_grad=False):
        """The hand-written backward pass of the LAST forward pass from the caller's d loss / d heat maps (pa_hg_set_heat_grads) instead
        of the built-in MSE gradient: any loss of the heat maps trains the net.  grad_outputs: a sequence of num_stacks fp32 GPU tensors
        [B][16][res/4][res/4] ('nchw', the shape forward() returns) or [B][res/4][res/4][16] ('nhwc'); None = zero for that stack.
        UNSCALED gradients (the engine applies _lib.grad_scale()); the parameter gradients land in flat_grads like loss_and_backward's,
        in phases with on_stack_done when an overlapping optimizer is attached.  A wrong count, shape, dtype or device raises ValueError
        before anything is launched.
        input_grad: True or 'nchw' also returns d loss / d image as a new fp32 tensor [B][3][res][res] (the shape of `x`), 'nhwc4' as
        [B][res][res][4] (img4's pixel order, 4th float 0): the gradient with respect to the image the forward pass read (x, or img4 as
        stored), unscaled -- one more launch, the data gradient of the 7x7 stride-2 stem.  False (default): None, no launch added.  Any
        other value raises ValueError."""
        lay = self._input_grad_layout(input_grad)
        require_gpu()
        if layout not in ('nchw', 'nhwc'):
            raise ValueError("layout must be 'nchw' or 'nhwc', got %r" % (layout,))
        grads = list(grad_outputs)
        if len(grads) != self.num_stacks:
            raise ValueError('backward: %d gradients for %d stacks' % (len(grads), self.num_stacks))
        if self._last_B is None:
            raise PoseAdvError('backward: no forward pass has run')
        B, Hh = self._last_B, self.res // 4
        want = (B, 16, Hh, Hh) if layout == 'nchw' else (B, Hh, Hh, 16)
        dev = self.flat_params.device
        for i, g in enumerate(grads):
            if g is None:
                continue
            if not torch.is_tensor(g) or tuple(g.shape) != want or g.dtype != torch.float32 or g.device != dev:
                raise ValueError('backward: gradient %d must be a float32 tensor %s on %s, got %s' % (
                    i, want, dev, '%s %s on %s' % (g.dtype, tuple(g.shape), g.device) if torch.is_tensor(g) else type(g).__name__))
        if all(g is None for g in grads):
            raise ValueError('backward: every gradient is None')
        h = self._net(B)
        keep = [None if g is None else g.contiguous() for g in grads]       # referenced until the call returns (read in stream order)
        for g in keep:
            if g is not None and g.data_ptr() % 16:
                raise ValueError('backward: gradients must be 16-byte aligned')
        ptrs = (C.c_void_p * self.num_stacks)(*[None if g is None else g.data_ptr() for g in keep])
        check(lib().pa_hg_set_heat_grads(h, ptrs, 0 if layout == 'nchw' else 1), 'pa_hg_set_heat_grads')
        dimg = None
        try:
            masks = self._set_masks(h, self._last_masks)        # the occlusion masks of that forward pass: the backward pass goes through them
            dimg = self._open_image_grad(h, B, lay)
            self._run_backward(h)
        finally:
            lib().pa_hg_set_heat_grads(h, None, 0)
            if lay is not None:
                lib().pa_hg_set_image_grad(h, None, 0)
            if self._last_masks is not None:
                self._set_masks(h, None)
        del keep, masks
        return dimg

    def forward_autograd(self, x=None, img4=None, pts=None, dropout_masks=None, layout='nchw'):
        """forward() whose per-stack heat maps carry a grad_fn: `loss = my_loss(outs); loss.backward(); optimizer.step()`.
        Returns a tuple of num_stacks tensors [B][16][res/4][res/4].  loss.backward() calls self.backward() once with the gradients autograd
        delivers; the parameter gradients land in flat_grads (the project's convention: the parameter views carry no .grad).  An input
        that requires grad gets its gradient like any autograd input: x.grad [B][3][res][res], or img4.grad (the NHWC4 gradient cast to
        img4's dtype, 4th channel 0) -- FGSM / PGD, a learnable occluder or a generator in front of the net; without requires_grad no
        launch is added.  The engine keeps ONE forward pass's activations: backward a second time through the same outputs, or after
        another forward pass of this net, raises RuntimeError.  pts is optional (accuracy() and _last_losses, as in forward());
        dropout_masks as in forward(): the backward pass differentiates through the same masks.
        layout='nhwc': the outputs are [B][res/4][res/4][16] views of the engine's own maps (heatmaps(layout='nhwc'): no conversion launch,
        valid until the next forward pass of this net), and the gradients autograd delivers go to backward(layout='nhwc') as they are --
        the layout pylib.Evaluation.soft_argmax(layout='nhwc') reads and writes in place."""
        if layout not in ('nchw', 'nhwc'):
            raise ValueError("layout must be 'nchw' or 'nhwc', got %r" % (layout,))
        self._ensure_table()
        if getattr(self, '_autograd_anchor', None) is None:
            self._autograd_anchor = torch.zeros(1, dtype=torch.float32, device=self.flat_params.device, requires_grad=True)
        return _HeatMapsFunction.apply(self._autograd_anchor, self, x, img4, pts, dropout_masks, layout)

    def accuracy(self, idxs, stack=-1):
        """Evaluation.accuracy (pylib/Evaluation.py:54-75) of the last forward's heat maps against the
        Gaussian target of the joints it was given, entirely on the device."""
        B = self._last_B
        h = self._net(B)
        stack = stack % self.num_stacks
        Hh = self.res // 4
        dev = self.flat_params.device
        scratch = torch.empty(B * 16 * Hh * Hh + 4 * B * 16 + B + 16, dtype=torch.float32, device=dev)
        # cached: a host->device copy here would make the host wait for the whole step (no run-ahead)
        key = tuple(int(i) for i in idxs)
        cache = self.__dict__.setdefault('_idx_cache', {})
        ix = cache.get(key)
        if ix is None:
            ix = cache[key] = torch.as_tensor(key, dtype=torch.int32, device=dev)
        acc = torch.empty(len(idxs) + 1, dtype=torch.float32, device=dev)          # pck_kernel writes every entry
        check(lib().pa_hg_accuracy(h, stack, ptr(ix), len(idxs), ptr(acc), ptr(scratch)), 'pa_hg_accuracy')
        if getattr(self, '_meter_keep', None) is not None:
            self._meter_keep += [scratch, acc, ix]
        return acc


    def pckh_origin_res(self, center, scale, rot, grnd_pts, normalizers, stack=-1, per_person=False):
        """Evaluation.accuracy_origin_res (pylib/Evaluation.py:77-97) -- and per_person_pckh (:99-167) when
        per_person -- of the last forward's heat maps, on the device.  Returns (acc[15], person[B] or None)."""
        from ..pylib.Evaluation import PCKH_JOINTS
        B = self._last_B
        h = self._net(B)
        stack = stack % self.num_stacks
        Hh = self.res // 4
        dev = self.flat_params.device
        if not hasattr(self, '_pckh_idx'):
            self._pckh_idx = torch.as_tensor(PCKH_JOINTS, dtype=torch.int32, device=dev)
        scratch = torch.empty(6 * B * 16 + (B * 16 * Hh * Hh if per_person else 0) + 16, dtype=torch.float32, device=dev)
        acc = torch.empty(len(PCKH_JOINTS) + 1, dtype=torch.float32, device=dev)
        person = torch.empty(B, dtype=torch.float32, device=dev) if per_person else None
        c = center.float().contiguous(); s = scale.float().contiguous(); r = rot.float().contiguous()
        g = grnd_pts.float().contiguous(); nm = normalizers.float().contiguous()
        check(lib().pa_hg_pckh(h, stack, ptr(c), ptr(s), ptr(r), ptr(g), ptr(nm), ptr(self._pckh_idx), len(PCKH_JOINTS),
                               ptr(acc), ptr(person), ptr(scratch)), 'pa_hg_pckh')
        if getattr(self, '_meter_keep', None) is not None:
            self._meter_keep += [scratch, acc, person, c, s, r, g, nm]
        return acc, person


def sample_mask(pred_masks, dropout_num=2, seed=0, step=0, uniforms=None):
    """_Hourglass._sample_mask (models/asn_stacked_hg.py:102-136) on the device: softmax over the 16 cells of each sample's
    [B][1][4][4] mask logits, `dropout_num` distinct cells drawn with those probabilities (the law of
    np.random.choice(replace=False); the engine's own counter-based stream, or `uniforms` [B][dropout_num] float64).
    Returns (masks [B][1][4][4] fp32 with zeros at the drawn cells, indexes [B][dropout_num] int64)."""
    assert pred_masks.dim() == 4 and pred_masks.shape[1] == 1 and pred_masks.shape[2] == pred_masks.shape[3]
    B, cells = pred_masks.shape[0], pred_masks.shape[2] * pred_masks.shape[3]
    dev = pred_masks.device
    lg = pred_masks.reshape(B, cells).float().contiguous()
    masks = torch.empty((B, cells), dtype=torch.float32, device=dev)
    idx = torch.empty((B, dropout_num), dtype=torch.int32, device=dev)
    u = uniforms.to(dev, torch.float64).contiguous() if uniforms is not None else None
    check(lib().pa_sample_dropout_masks(ptr(lg), B, cells, dropout_num, int(seed), int(step), ptr(u), None, ptr(masks), ptr(idx),
                                        stream()), 'pa_sample_dropout_masks')
    return masks.view(pred_masks.shape), idx.long()


def dropout(x, masks):
    """_Hourglass._dropout (models/asn_stacked_hg.py:79-100) on an NCHW fp32 tensor (operator-level entry; the networks apply
    it inside pa_hg_forward): the [B][1][4][4] cell mask, nearest-upsampled to the map, times every channel."""
    B, Cc, H, W = x.shape
    pad = (-Cc) % 8
    xh = torch.nn.functional.pad(x.permute(0, 2, 3, 1), (0, pad)).to(_lib.act_dtype()).contiguous()
    out = torch.empty_like(xh)
    m = masks.to(x.device, torch.float32).reshape(B, 16).contiguous()
    check(lib().pa_cell_mask(ptr(xh), ptr(m), ptr(out), B, H, W, Cc + pad, stream()), 'pa_cell_mask')
    return out[..., :Cc].permute(0, 3, 1, 2).float()


def create_hg(num_stacks, num_modules, num_classes, chan, res=256, default_batch=24):
    """models/asn_stacked_hg.py:344-347."""
    return HourglassNet(num_modules=num_modules, num_stacks=num_stacks, chan=chan, num_classes=num_classes,
                        res=res, default_batch=default_batch)


def create_asn(chan_in, chan_out, scale_num=None, rotation_num=None, is_aug=False, is_dropout=False, res=256,
               default_batch=24):
    """models/asn_stacked_hg.py:441-444: the scale/rotation agent (is_aug) or the occlusion agent (is_dropout)."""
    from .asn import ASN
    assert is_aug != is_dropout                              # :351
    if chan_in != chan_out:
        raise ValueError('the reference always builds the agent with chan_in == chan_out')
    return ASN(chan_out, scale_num, rotation_num, res=res, default_batch=default_batch, is_dropout=is_dropout)
