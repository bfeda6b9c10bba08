"""Optimizers on the engine's flat parameter buffer, with the data-parallel gradient exchange folded in: ONE all-reduce of the flat
gradient over RCCL per step (replaces nn.DataParallel's broadcast/gather/reduce_add, stack-hg.py:49).

RMSprop (reference: torch.optim.RMSprop(net.parameters(), lr, alpha=0.99, eps=1e-8, momentum=0, weight_decay=0), stack-hg.py:51-52).
Beyond the reference's recipe: torch.optim.RMSprop's momentum, weight_decay and centered, and the gradient-norm clipping of
torch.nn.utils.clip_grad_norm_ (max_grad_norm), all inside the engine's own launches (pa_rmsprop_step_opts, pa_grad_norm).  With
every one of them off, step() is the one pa_rmsprop_step_state call it has always been.

Adam / AdamW (torch.optim.Adam's formula with weight decay coupled or decoupled, AMSGrad, the same clipping): one fused step
(pa_adam_step) whose step count and bias-correction constants live on the device.  make_optimizer picks one from the command line.

SGD / LARS / LAMB: torch.optim.SGD (momentum, Nesterov), and the two optimizers for large batches that scale every tensor's step by
||w|| / ||update|| on the device (pa_lars_step, pa_lamb_step: a segmented per-tensor reduction, no host synchronisation).

ModelEma: an exponential moving average of the weights in a twin net, updated on the device behind the step (pa_ema_advance, pa_ema_lerp);
its update count and the decision to hold on a skipped step live on the device, next to the optimizer's flag.  make_ema: from the command line.

Gradient accumulation: optimizer.accumulate() after a backward pass instead of step() folds flat_grads into a private sum
(pa_grad_accumulate); the step() that ends the group adds the sum to its own gradient and takes the mean through gscale.
accum_plan: which iterations of an epoch step (--accum_steps)."""
import ctypes as C
import os

import torch
import torch.distributed as dist

from .. import _lib
from .._lib import lib, check, ptr, stream


def _dist_on():
    """Gradients go through the process group: world > 1, or a single rank forced through it (POSEADV_FORCE_DIST=1: RCCL
    on a one-GPU box, tests/test_gpu_rccl.py)."""
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get('POSEADV_FORCE_DIST') == '1')


def optim_options(opt):
    """RMSprop keyword arguments from the command line (options/train_options.py: --momentum --weight_decay --centered
    --clip_grad_norm, 0 = off)"""
    clip = float(getattr(opt, 'clip_grad_norm', 0) or 0)
    return dict(momentum=float(getattr(opt, 'momentum', 0) or 0), weight_decay=float(getattr(opt, 'weight_decay', 0) or 0),
                centered=bool(getattr(opt, 'centered', 0)), max_grad_norm=clip if clip > 0 else None)


class _FlatOptimizer(object):
    """What every optimizer on the engine's flat arrays does around its own step launch: the gradient exchange (one all-reduce, or the
    overlapped per-stack buckets), gscale, the gradient norm and clip coefficient on the device, and the refresh of the 16-bit weight
    copies after the step."""
    def _attach(self, net, max_grad_norm, overlap):
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError('max_grad_norm must be > 0 (None: no clipping)')
        self.net = net
        self._works, self._comm, self._ranges = [], None, {}
        if overlap and hasattr(net, 'num_stacks'):
            net.on_stack_done = self._exchange_stack
        net._ensure_table()
        self.max_grad_norm = max_grad_norm
        self._norm_ws = self._norm_out = None           # the norm's scratch and its {norm, coefficient} output
        self._clipped = False
        # gradient accumulation: the fp32 sum of the micro-batch gradients since the last step (allocated by the first accumulate()), and
        # how many it holds
        self._overlap, self._acc, self.pending = bool(overlap), None, 0

    def zero_grad(self):
        """also drops a pending group of accumulate() calls"""
        self.net.zero_grad()
        self.pending = 0

    def accumulate(self):
        """Call after a backward pass INSTEAD of step(): this micro-batch's flat_grads joins the sum of its group (every backward pass
        overwrites flat_grads; two of them before a step() do not add up by themselves, as torch's .grad does).  The first of a group
        is a copy, the later ones _acc = _acc + flat_grads: one launch of pa_grad_accumulate, fp32, in the order of the calls.  The step()
        that ends the group adds _acc to its own gradient and divides by the group's size (_exchanged_gscale); the gradient is exchanged
        between ranks there, once per group.  BatchNorm statistics stay per micro-batch."""
        if self._overlap:
            raise ValueError('accumulate() on an optimizer created with overlap=True: its per-stack buckets would exchange the gradient '
                             'of every micro-batch; create the optimizer with overlap=False')
        grads = self.net.flat_grads
        if self._acc is None:
            self._acc = torch.empty_like(grads)
        first = self.pending == 0
        check(lib().pa_grad_accumulate(ptr(self._acc), ptr(grads if first else self._acc), None if first else ptr(grads), grads.numel(), stream()),
              'pa_grad_accumulate')
        self.pending += 1

    def _warn_pending(self):
        if self.pending:
            import warnings
            warnings.warn('state_dict(): %d accumulated micro-batch gradient(s) are pending and are NOT saved; call step() first' % self.pending)

    def allreduce_grads(self):
        """Sum the flat gradient over all ranks (RCCL when the process group backend is nccl)."""
        if _dist_on():
            dist.all_reduce(self.net.flat_grads, op=dist.ReduceOp.SUM)
            return 1.0 / dist.get_world_size()
        return 1.0

    def _exchange_stack(self, stack):
        """hook of HourglassNet.loss_and_backward: the backward pass of `stack` has just been enqueued"""
        if not _dist_on():
            return
        net = self.net
        h = net._net(net._last_B)
        if stack not in self._ranges:
            lo, hi = C.c_size_t(), C.c_size_t()
            check(lib().pa_hg_bucket_range(h, stack, C.byref(lo), C.byref(hi)), 'pa_hg_bucket_range')
            self._ranges[stack] = (lo.value, hi.value)
        if self._comm is None:
            self._comm = torch.cuda.Stream()
            net.flat_grads.record_stream(self._comm)
        rc = lib().pa_hg_bucket_wait(h, stack, C.c_void_p(self._comm.cuda_stream))
        if rc == -1:
            return                                   # this stream mode finishes gradients at the end only
        check(rc, 'pa_hg_bucket_wait')
        lo, hi = self._ranges[stack]
        with torch.cuda.stream(self._comm):          # the collective is ordered behind the bucket event on this stream
            work = dist.all_reduce(net.flat_grads[lo:hi], op=dist.ReduceOp.SUM, async_op=True)
        self._works.append((lo, hi, work))

    def _finish_exchange(self):
        """the ranges no bucket covered, then wait for the buckets in flight"""
        n = self.net.flat_grads.numel()
        done = sorted((lo, hi) for lo, hi, _ in self._works)
        pos = 0
        for lo, hi in done + [(n, n)]:
            if lo > pos:
                dist.all_reduce(self.net.flat_grads[pos:lo], op=dist.ReduceOp.SUM)
            pos = max(pos, hi)
        for _, _, work in self._works:
            work.wait()                              # the current stream waits for the collective
        self._works = []
        return 1.0 / dist.get_world_size()

    def _exchanged_gscale(self):
        """finish the gradient exchange; 1/world, and the fp16 build's gradient scale divided out.  With k micro-batches pending
        (accumulate()): first flat_grads = _acc + flat_grads, so that the exchange, the norm, the step and the fp16 build's finite check
        read the group's sum where they read every gradient, and the mean over the k + 1 goes into gscale."""
        k = self.pending
        if k:
            grads = self.net.flat_grads
            check(lib().pa_grad_accumulate(ptr(grads), ptr(self._acc), ptr(grads), grads.numel(), stream()), 'pa_grad_accumulate')
        world_scale = self._finish_exchange() if self._works else self.allreduce_grads()
        gscale = world_scale / _lib.grad_scale()
        if k:
            gscale, self.pending = gscale / (k + 1), 0
        return gscale

    def _clip_coef(self, n, gscale, frozen=0):
        """norm and clip coefficient of the exchanged gradient (max_grad_norm): the pointer of the device float the step reads, or None.
        frozen: the bit mask of the frozen parameter groups, whose chunks the norm leaves out (pa_grad_norm_groups)"""
        if self.max_grad_norm is None:
            return None
        grads = self.net.flat_grads
        if self._norm_out is None:
            self._norm_ws = torch.empty(int(lib().pa_grad_norm_workspace_bytes(n)) // 8, dtype=torch.float64, device=grads.device)
            self._norm_out = torch.zeros(2, dtype=torch.float32, device=grads.device)
        if frozen:
            check(lib().pa_grad_norm_groups(ptr(grads), n, ptr(self._map), int(frozen), float(gscale), float(self.max_grad_norm),
                                            ptr(self._norm_ws), ptr(self._norm_out), stream()), 'pa_grad_norm_groups')
        else:
            check(lib().pa_grad_norm(ptr(grads), n, float(gscale), float(self.max_grad_norm), ptr(self._norm_ws), ptr(self._norm_out), stream()),
                  'pa_grad_norm')
        self._clipped = True
        return ptr(self._norm_out[1:])

    def _weights_stepped(self):
        self.net.weights_changed()
        self.net._net(self.net._last_B or self.net.default_batch)      # refresh the bf16 weight copies now

    def last_grad_norm(self):
        """The norm of the (averaged, unscaled) gradient of the last step taken with max_grad_norm, before clipping, over the
        parameter groups that are not frozen: a 0-dim tensor on the device, so reading it is the caller's synchronisation (at print time); None before the first such step."""
        return self._norm_out[0] if self._clipped else None

    def _params(self):
        """(name, shape, offset, numel, kind) of the parameters, in parameters() order"""
        return [t for t in self.net._table if t[4] == 0]

    # ---- parameter groups
    def _init_groups(self, base, groups):
        """self.param_groups from the constructor's options `base` and its `groups` argument.  None: the one group there has always
        been, with exactly the keys it has always had, and no call of this class changes.  A list of specs {'params': selector, 'lr',
        'weight_decay', 'frozen', 'lr_mult'}: param_groups[0] is the default group (what no spec takes, base's lr and weight_decay), spec
        k is param_groups[k + 1]; every group is a dict with all option keys, 'frozen', 'lr_mult', 'params' (indices in parameters()
        order) and 'names'.  The first spec that matches a parameter takes it.  The chunk map (pa_opt_chunk_map_host on the net's
        table) is built and uploaded here, once."""
        self._map = self._group_consts = None
        self._shared = tuple(k for k in base if k not in ('lr', 'weight_decay'))
        if groups is None:
            self.param_groups = [base]
            return
        params = self._params()
        names = [t[0] for t in params]
        specs = list(groups)
        if len(specs) + 1 > _lib.OPT_GROUPS_MAX:
            raise ValueError('%d parameter groups (the default group and %d specs): at most %d' % (len(specs) + 1, len(specs), _lib.OPT_GROUPS_MAX))
        owner = [0] * len(params)
        taken = [False] * len(params)
        for k, spec in enumerate(specs):
            unknown = set(spec) - set(('params', 'lr', 'weight_decay', 'frozen', 'lr_mult'))
            if 'params' not in spec or unknown:
                raise ValueError("group %d: a spec is {'params': selector, 'lr', 'weight_decay', 'frozen', 'lr_mult'}; got keys %s" % (k, sorted(spec)))
            hit = _select(spec['params'], params)
            if not any(hit):
                raise ValueError('group %d: the selector %r matches no parameter' % (k, spec['params']))
            for i, h in enumerate(hit):
                if h and not taken[i]:
                    owner[i], taken[i] = k + 1, True
        base_lr = float(base['lr'])
        self.param_groups = []
        for k, spec in enumerate([{}] + specs):
            g = dict(base)
            if 'lr' in spec and 'lr_mult' in spec:
                raise ValueError("group %d: give 'lr' or 'lr_mult', not both" % (k - 1))
            if 'lr' in spec:
                g['lr'] = spec['lr']
                g['lr_mult'] = float(spec['lr']) / base_lr if base_lr != 0 else 1.0
            else:
                g['lr_mult'] = float(spec.get('lr_mult', 1.0))
                if 'lr_mult' in spec:
                    g['lr'] = base_lr * g['lr_mult']
            if not float(g['lr']) >= 0 or not g['lr_mult'] >= 0:
                raise ValueError('group %d: lr and lr_mult must be >= 0' % (k - 1))
            g['weight_decay'] = spec.get('weight_decay', base['weight_decay'])
            if not float(g['weight_decay']) >= 0:
                raise ValueError('group %d: weight_decay must be >= 0' % (k - 1))
            g['frozen'] = bool(spec.get('frozen', False))
            g['params'] = [i for i in range(len(params)) if owner[i] == k]
            g['names'] = [names[i] for i in g['params']]
            self.param_groups.append(g)
        n = self.net.flat_params.numel()
        nt = len(params)
        offsets = (C.c_size_t * nt)(*[t[2] for t in params])
        numels = (C.c_size_t * nt)(*[t[3] for t in params])
        group = (C.c_int32 * nt)(*owner)
        host = (C.c_uint8 * ((n + 3) // 4))()
        check(lib().pa_opt_chunk_map_host(offsets, numels, group, nt, n, len(self.param_groups), host), 'pa_opt_chunk_map_host')
        dev = self.net.flat_params.device
        self._map = torch.frombuffer(host, dtype=torch.uint8).clone().to(dev)
        self._group_consts = torch.zeros(_lib.OPT_GROUPS_MAX, dtype=torch.float32, device=dev)      # Adam: lr_k / bc1 of the last taken step

    def _grouped(self):
        return self._map is not None

    def _group_table(self):
        """(pa_opt_group array, ngroups, 16-bit mask of the frozen groups) from param_groups as they are NOW; the shared options are
        group 0's, and another group's copy that differs is an error"""
        gs = self.param_groups
        if len(gs) > _lib.OPT_GROUPS_MAX:
            raise ValueError('%d parameter groups: at most %d' % (len(gs), _lib.OPT_GROUPS_MAX))
        for k, g in enumerate(gs[1:], 1):
            for key in self._shared:
                a, b = g.get(key), gs[0].get(key)
                if (tuple(a) if isinstance(a, (list, tuple)) else a) != (tuple(b) if isinstance(b, (list, tuple)) else b):
                    raise ValueError('param_groups[%d][%r] = %r differs from param_groups[0][%r] = %r: %s is shared by all groups '
                                     '(only lr, weight_decay and frozen are per group)' % (k, key, a, key, b, key))
        tab = (_lib.OptGroup * len(gs))()
        mask = 0
        for k, g in enumerate(gs):
            tab[k].lr, tab[k].weight_decay, tab[k].frozen = float(g['lr']), float(g.get('weight_decay', 0)), int(bool(g.get('frozen', False)))
            mask |= tab[k].frozen << k
        return tab, len(gs), mask

    def _frozen_params(self):
        """indices (parameters() order) of the parameters in a frozen group"""
        return set(i for g in self.param_groups if g.get('frozen', False) for i in g.get('params', ()))

    # ---- per-tensor work (SGD / LARS / LAMB)
    def _init_segments(self):
        """The segment list of the flat parameter array (pa_opt_segments_host on the net's table, with the group of every tensor), built
        and uploaded here, once; the workspace of the per-tensor sums, the norms [2][ntensors] and the trust ratios (1 until a step
        writes them), in _params() order."""
        params = self._params()
        nt, n = len(params), self.net.flat_params.numel()
        owner = [0] * nt
        for k, g in enumerate(self.param_groups):
            for i in g.get('params', ()):
                owner[i] = k
        offsets = (C.c_size_t * nt)(*[t[2] for t in params])
        numels = (C.c_size_t * nt)(*[t[3] for t in params])
        group = (C.c_int32 * nt)(*owner)
        count = int(lib().pa_opt_segments_host(offsets, numels, group, nt, n, None, 0))
        if count == 0:
            check(1, 'pa_opt_segments_host')
        host = (_lib.OptSegment * count)()
        if int(lib().pa_opt_segments_host(offsets, numels, group, nt, n, host, count)) != count:
            check(1, 'pa_opt_segments_host')
        dev = self.net.flat_params.device
        self._segs = torch.frombuffer(host, dtype=torch.int32).clone().to(dev)
        self._nsegs, self._ntensors = count, nt
        self._layer_ws = torch.empty(int(lib().pa_opt_layer_workspace_bytes(count, nt)) // 8, dtype=torch.float64, device=dev)
        self._norms = torch.zeros(2 * nt, dtype=torch.float32, device=dev)
        self._trust = torch.ones(nt, dtype=torch.float32, device=dev)
        self._trusted = False

    def last_trust(self):
        """The trust ratio r_t of every parameter at the last step, in _params() order (1 for a tensor that is not adapted, the value
        of the last step taken for a frozen one): a device tensor, so reading it is the caller's synchronisation.  None before the
        first step, and for SGD without trust."""
        return self._trust if getattr(self, '_trusted', False) else None

    def tensor_norms(self):
        """(||w||, ||update|| or ||gradient||) per parameter at the last step, the weights BEFORE it: two device tensors of one float
        per parameter, in _params() order.  None when last_trust() is."""
        nt = self._ntensors
        return (self._norms[:nt], self._norms[nt:]) if getattr(self, '_trusted', False) else None

    def describe_groups(self):
        """one line per parameter group for the log: tensors, floats, lr, weight_decay, frozen"""
        params = self._params()
        lines = []
        for k, g in enumerate(self.param_groups):
            idx = g.get('params', range(len(params)))
            lines.append('param group %d: %d tensors, %d floats, lr %g, weight_decay %g, frozen %d' % (
                k, len(idx), sum(params[i][3] for i in idx), g['lr'], g.get('weight_decay', 0), int(bool(g.get('frozen', False)))))
        return lines

    def _state_groups(self):
        """state_dict()'s 'param_groups': torch's format, the 'params' lists partition 0 .. P - 1"""
        out = []
        for g in self.param_groups:
            pg = dict(g)
            if 'betas' in pg:
                pg['betas'] = tuple(pg['betas'])
            pg['params'] = list(g['params']) if 'params' in g else list(range(len(self._params())))
            if 'names' in pg:
                pg['names'] = list(pg['names'])
            out.append(pg)
        return out

    def _file_keys(self, sd):
        """The file's state keys in parameters() order, and whether its groups partition the parameters as this optimizer's do.  The
        ids of a file are positions in ITS chained group order (torch numbers them so; this class's own files use the parameter
        index, which is the same thing read through the groups' 'params' lists).  Same group sizes: position j of the file's chain is
        position j of this optimizer's chain.  Otherwise: position j of the file is parameter j.
        A file of this class with several groups says which parameters each group holds ('names', and its ids ARE parameter indices):
        its membership is compared exactly, and where it differs the state still goes to the parameter each id names."""
        nparams = len(self._params())
        fgs = sd['param_groups']
        chain = [key for fg in fgs for key in fg.get('params', [])] if all('params' in fg for fg in fgs) else list(range(nparams))
        if len(chain) != nparams:
            return None, False
        mine = [list(g['params']) if 'params' in g else list(range(nparams)) for g in self.param_groups]
        if all('names' in fg and 'params' in fg for fg in fgs) and sorted(chain) == list(range(nparams)):
            names = [t[0] for t in self._params()]
            same = len(fgs) == len(mine) and all(list(fg['params']) == m and list(fg['names']) == [names[i] for i in m] for fg, m in zip(fgs, mine))
            return list(range(nparams)), same
        if [len(fg.get('params', chain)) for fg in fgs] == [len(m) for m in mine]:
            keys = [None] * nparams
            for key, i in zip(chain, [i for m in mine for i in m]):
                keys[i] = key
            return keys, True
        return chain, False

    def _load_groups(self, sd, matched, shared_keys):
        """the group options of a file.  A file with this optimizer's partition: lr, weight_decay, frozen, lr_mult per group.  Any
        other file into a grouped optimizer: the per-group values stay this optimizer's (one warning).  The shared options come from
        the file's group 0 either way, into every group."""
        fgs = sd['param_groups']
        shared = dict((k, v) for k, v in fgs[0].items() if k in shared_keys)
        if 'betas' in shared:
            shared['betas'] = tuple(shared['betas'])
        for g in self.param_groups:
            g.update(shared)
        if matched:
            for g, fg in zip(self.param_groups, fgs):
                for k in ('lr', 'weight_decay') + (('frozen', 'lr_mult') if self._grouped() else ()):
                    if k in fg:
                        g[k] = fg[k]
        else:
            import warnings
            warnings.warn('optimizer state: the file has %d parameter group(s) that do not partition the parameters as the %d of this '
                          'optimizer do: the state is loaded by position and the shared options from its group 0; every group keeps its '
                          'own lr, weight_decay, frozen and lr_mult' % (len(fgs), len(self.param_groups)))


def _select(selector, params):
    """which of `params` ((name, shape, ...) in parameters() order) a group selector takes: a regular expression (re.search on the
    state-dict name), a callable (name, shape) -> bool, or a list of names (each must exist)"""
    if callable(selector):
        return [bool(selector(t[0], tuple(t[1]))) for t in params]
    if isinstance(selector, str):
        import re
        rx = re.compile(selector)
        return [rx.search(t[0]) is not None for t in params]
    wanted = set(selector)
    unknown = sorted(wanted - set(t[0] for t in params))
    if unknown:
        raise ValueError('group selector names parameters that do not exist: %s' % ', '.join(unknown))
    return [t[0] in wanted for t in params]


def no_decay_1d(name, shape):
    """group selector: the tensors with ndim <= 1 (BatchNorm weight and bias, conv and linear biases), which an AdamW recipe does not decay"""
    return len(shape) <= 1


class RMSprop(_FlatOptimizer):
    def __init__(self, net, lr=2.5e-4, alpha=0.99, eps=1e-8, momentum=0, weight_decay=0, centered=False, max_grad_norm=None, overlap=False,
                 groups=None):
        """momentum, weight_decay, centered: torch.optim.RMSprop's (torch 2.10 _single_tensor_rmsprop), except that the centered
        variance max(0, square_avg - grad_avg^2) is clamped where torch returns NaN for a difference that rounding made negative.
        They live in param_groups[0] and are read at every step, like lr.  max_grad_norm (None = off): the gradient is multiplied by
        min(1, max_grad_norm / (norm + 1e-6)) as by torch.nn.utils.clip_grad_norm_; the norm is computed on the device and the step
        reads the coefficient there (no host synchronisation); last_grad_norm() is the device float for logging.
        overlap (pose net, world > 1 only): exchange the gradients of a stack's hourglass (one contiguous 42 % of a 2-stack
        net) on a communication stream as soon as that stack's backward pass is enqueued, while the earlier stacks and the stem
        still run; the rest follows at the end.  Same sums, same result as the single all-reduce (off by default).
        groups (None: one group, everything as ever): parameter groups with their own lr / weight_decay / frozen, see _init_groups;
        every step then goes through pa_rmsprop_step_groups, and the norm through pa_grad_norm_groups when a group is frozen."""
        if momentum < 0 or weight_decay < 0:
            raise ValueError('momentum and weight_decay must be >= 0')
        self._attach(net, max_grad_norm, overlap)
        self._init_groups({'lr': lr, 'alpha': alpha, 'eps': eps, 'momentum': momentum, 'weight_decay': weight_decay, 'centered': bool(centered)}, groups)
        self.square_avg = torch.zeros_like(net.flat_params)
        # flat like square_avg, allocated when their option is on (_ensure_state)
        self.momentum_buffer = self.grad_avg = None
        self._ensure_state(self.param_groups[0])
        # fp16 build: {this gradient is non-finite, steps skipped so far} of THIS optimizer (the pose net's and the agent's step on
        # different streams in the joint stage; a process-wide flag would let one see the other's overflow)
        self._skip_state = torch.zeros(2, dtype=torch.int32, device=net.flat_params.device)
        self.steps = 0

    def _ensure_state(self, g):
        """momentum_buffer / grad_avg of the options that are on in the param group g (zeros, as torch creates them at the first step)"""
        if g.get('momentum', 0) > 0 and self.momentum_buffer is None:
            self.momentum_buffer = torch.zeros_like(self.net.flat_params)
        if g.get('centered', False) and self.grad_avg is None:
            self.grad_avg = torch.zeros_like(self.net.flat_params)

    def step(self):
        g = self.param_groups[0]
        gscale = self._exchanged_gscale()
        n = self.net.flat_params.numel()
        mom, wd, centered = float(g.get('momentum', 0)), float(g.get('weight_decay', 0)), bool(g.get('centered', False))
        if self._grouped():
            self._step_groups(g, mom, centered, n, gscale)
        elif mom == 0 and wd == 0 and not centered and self.max_grad_norm is None:          # the reference's recipe: one launch, as ever
            check(lib().pa_rmsprop_step_state(ptr(self.net.flat_params), ptr(self.net.flat_grads), ptr(self.square_avg), n,
                                              float(g['lr']), float(g['alpha']), float(g['eps']), float(gscale), ptr(self._skip_state), stream()),
                  'pa_rmsprop_step_state')
        else:
            self._step_opts(g, mom, wd, centered, n, gscale)
        self.steps += 1
        self._weights_stepped()

    def _step_opts(self, g, mom, wd, centered, n, gscale):
        """norm and clip coefficient of the exchanged gradient (max_grad_norm), then the step that reads the coefficient on the device"""
        self._ensure_state(g)
        grads, coef = self.net.flat_grads, self._clip_coef(n, gscale)
        o = _lib.RmspropOpts(float(g['lr']), float(g['alpha']), float(g['eps']), mom, wd, int(centered))
        check(lib().pa_rmsprop_step_opts(C.byref(o), ptr(self.net.flat_params), ptr(grads), ptr(self.square_avg),
                                         ptr(self.momentum_buffer) if mom > 0 else None, ptr(self.grad_avg) if centered else None,
                                         n, float(gscale), coef, ptr(self._skip_state), stream()), 'pa_rmsprop_step_opts')

    def _step_groups(self, g, mom, centered, n, gscale):
        """the step with parameter groups: lr, weight_decay and frozen of every group as they are now, the other options group 0's"""
        tab, ngroups, frozen = self._group_table()
        self._ensure_state(g)
        coef = self._clip_coef(n, gscale, frozen)
        o = _lib.RmspropOpts(float(g['lr']), float(g['alpha']), float(g['eps']), mom, 0.0, int(centered))
        check(lib().pa_rmsprop_step_groups(C.byref(o), tab, ngroups, ptr(self._map), ptr(self.net.flat_params), ptr(self.net.flat_grads),
                                           ptr(self.square_avg), ptr(self.momentum_buffer) if mom > 0 else None,
                                           ptr(self.grad_avg) if centered else None, n, float(gscale), coef, ptr(self._skip_state), stream()),
              'pa_rmsprop_step_groups')

    def skip_flag_ptr(self):
        """device address of the int32 "the last step was skipped" flag (ModelEma.update reads it on the device)"""
        return ptr(self._skip_state)

    def skipped_steps(self):
        """fp16 build: optimizer steps the engine skipped because the (scaled) gradient held inf / NaN; 0 in the bf16 build"""
        n = C.c_longlong(0)
        check(lib().pa_rmsprop_skipped_steps_state(ptr(self._skip_state), C.byref(n), stream()), 'pa_rmsprop_skipped_steps_state')
        return int(n.value)

    def _option_state(self, g):
        self._ensure_state(g)
        return ([('momentum_buffer', self.momentum_buffer)] if g.get('momentum', 0) > 0 else []) + \
            ([('grad_avg', self.grad_avg)] if g.get('centered', False) else [])

    # torch.optim-compatible (de)serialisation: per-parameter state keyed by index, in parameters() order
    def state_dict(self):
        self._warn_pending()
        state = {}
        for i, (name, shape, off, numel, kind) in enumerate(t for t in self.net._table if t[4] == 0):
            state[i] = {'step': self.steps, 'square_avg': self.square_avg[off:off + numel].view(shape).clone()}
            for key, flat in self._option_state(self.param_groups[0]):          # torch's keys, present when the option is on
                state[i][key] = flat[off:off + numel].view(shape).clone()
        return {'state': state, 'param_groups': self._state_groups()}

    def load_state_dict(self, sd):
        """Accepts this class's own files and torch.optim.RMSprop's: `state` is keyed by the entries of
        param_groups[0]['params'] (positions 0..n-1 in current torch, object ids in the reference's torch 0.3), in
        parameters() order either way.  A missing or mis-shaped entry is reported, never silently dropped.  momentum_buffer and
        grad_avg are read when the file's param group (else this optimizer's) has the option on; a file without them (written with
        the option off) leaves them zero, with a warning."""
        import warnings
        params = self._params()
        group = dict(self.param_groups[0])
        group.update((k, v) for k, v in sd['param_groups'][0].items() if k != 'params')
        extra = self._option_state(group)
        loaded = dict((key, 0) for key, _ in extra)
        for _, flat in extra:
            flat.zero_()
        state = sd.get('state', {})
        keys, matched = self._file_keys(sd)
        if keys is None:
            warnings.warn('optimizer state has %d parameters, the network %d: square_avg not loaded'
                          % (sum(len(fg.get('params', [])) for fg in sd['param_groups']), len(params)))
            keys = []
        missing = 0
        frozen = self._frozen_params()
        for i, (key, (name, shape, off, numel, kind)) in enumerate(zip(keys, params)):
            st = state.get(key)
            if st is None and i in frozen:              # (torch keeps no state for a parameter it never stepped)
                for ekey in loaded:
                    loaded[ekey] += 1
                continue
            if st is None or 'square_avg' not in st:
                missing += 1
                continue
            v = torch.as_tensor(st['square_avg'])
            if v.numel() != numel:
                warnings.warn('optimizer state of %s has %d elements, expected %d: skipped' % (name, v.numel(), numel))
                missing += 1
                continue
            self.square_avg[off:off + numel] = v.reshape(-1).to(self.square_avg.device, torch.float32)
            self.steps = int(st.get('step', self.steps))
            for ekey, flat in extra:
                e = st.get(ekey)
                if e is not None and torch.as_tensor(e).numel() == numel:
                    flat[off:off + numel] = torch.as_tensor(e).reshape(-1).to(flat.device, torch.float32)
                    loaded[ekey] += 1
        for ekey, _ in extra:
            if loaded[ekey] < len(params):
                warnings.warn('optimizer state: %d of %d parameters had no %s entry (left at zero)' % (len(params) - loaded[ekey], len(params), ekey))
        if missing and state:
            warnings.warn('optimizer state: %d of %d parameters had no square_avg entry (left at their current value)' % (missing, len(params)))
        if not self._grouped() and len(sd['param_groups']) == 1:
            for k, v in sd['param_groups'][0].items():
                if k != 'params':
                    self.param_groups[0][k] = v
        else:
            self._load_groups(sd, matched, self._shared)


_ADAM_KEYS = ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'decoupled_weight_decay')


class Adam(_FlatOptimizer):
    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, decoupled_weight_decay=False,
                 max_grad_norm=None, overlap=False, groups=None):
        """torch.optim.Adam (torch 2.10 _single_tensor_adam) as one fused step on the flat arrays (pa_adam_step): weight_decay coupled
        (added to the gradient) or, with decoupled_weight_decay, AdamW's p *= 1 - lr weight_decay; amsgrad keeps the running maximum
        of exp_avg_sq (max_exp_avg_sq, allocated when amsgrad is first on).  All of them live in param_groups[0] and are read at every
        step, like lr.  max_grad_norm, overlap and groups: as for RMSprop (pa_adam_step_groups; the step sizes lr_k / bc1 of the groups
        live in self._group_consts on the device).
        The step count of the bias correction lives on the device (self._state, a pa_adam_state): the fp16 build decides there whether
        a step is taken, and a skipped step must not advance it.  steps_taken() and state_dict() read it, which synchronises."""
        b1, b2 = betas
        if not (0 <= b1 < 1 and 0 <= b2 < 1):
            raise ValueError('betas must be in [0, 1)')
        if not eps > 0 or weight_decay < 0:
            raise ValueError('eps must be > 0 and weight_decay >= 0')
        self._attach(net, max_grad_norm, overlap)
        self._init_groups({'lr': lr, 'betas': (b1, b2), 'eps': eps, 'weight_decay': weight_decay, 'amsgrad': bool(amsgrad),
                           'decoupled_weight_decay': bool(decoupled_weight_decay)}, groups)
        self.exp_avg = torch.zeros_like(net.flat_params)
        self.exp_avg_sq = torch.zeros_like(net.flat_params)
        self.max_exp_avg_sq = None
        self._ensure_state(self.param_groups[0])
        # pa_adam_state: {flag, skipped, step, reserved} int32 and {bc1, bc2, step_size, bc2s} float32 of THIS optimizer
        self._state = torch.zeros(8, dtype=torch.int32, device=net.flat_params.device)

    def _ensure_state(self, g):
        if g.get('amsgrad', False) and self.max_exp_avg_sq is None:
            self.max_exp_avg_sq = torch.zeros_like(self.net.flat_params)

    def step(self):
        g = self.param_groups[0]
        gscale = self._exchanged_gscale()
        n = self.net.flat_params.numel()
        amsgrad = bool(g.get('amsgrad', False))
        self._ensure_state(g)
        b1, b2 = g['betas']
        o = _lib.AdamOpts(float(g['lr']), float(b1), float(b2), float(g['eps']), float(g.get('weight_decay', 0)), int(amsgrad),
                          int(bool(g.get('decoupled_weight_decay', False))))
        if self._grouped():
            tab, ngroups, frozen = self._group_table()
            coef = self._clip_coef(n, gscale, frozen)
            check(lib().pa_adam_step_groups(C.byref(o), tab, ngroups, ptr(self._map), ptr(self._group_consts), ptr(self.net.flat_params),
                                            ptr(self.net.flat_grads), ptr(self.exp_avg), ptr(self.exp_avg_sq),
                                            ptr(self.max_exp_avg_sq) if amsgrad else None, n, float(gscale), coef, ptr(self._state), stream()),
                  'pa_adam_step_groups')
            self._weights_stepped()
            return
        coef = self._clip_coef(n, gscale)
        check(lib().pa_adam_step(C.byref(o), ptr(self.net.flat_params), ptr(self.net.flat_grads), ptr(self.exp_avg), ptr(self.exp_avg_sq),
                                 ptr(self.max_exp_avg_sq) if amsgrad else None, n, float(gscale), coef, ptr(self._state), stream()),
              'pa_adam_step')
        self._weights_stepped()

    def _counts(self):
        steps, skipped = C.c_longlong(0), C.c_longlong(0)
        check(lib().pa_adam_steps(ptr(self._state), C.byref(steps), C.byref(skipped), stream()), 'pa_adam_steps')
        return int(steps.value), int(skipped.value)

    def skip_flag_ptr(self):
        """device address of the int32 "the last step was skipped" flag, word 0 of the pa_adam_state (ModelEma.update reads it on the device)"""
        return ptr(self._state)

    def steps_taken(self):
        """optimizer steps applied so far (skipped ones not counted), read from the device: synchronises the stream"""
        return self._counts()[0]

    def skipped_steps(self):
        """fp16 build: optimizer steps the engine skipped because the (scaled) gradient held inf / NaN; 0 in the bf16 build"""
        return self._counts()[1]

    def _moments(self, g):
        self._ensure_state(g)
        return [('exp_avg', self.exp_avg), ('exp_avg_sq', self.exp_avg_sq)] + ([('max_exp_avg_sq', self.max_exp_avg_sq)] if g.get('amsgrad', False) else [])

    # torch.optim.Adam's format: per-parameter state keyed by index, in parameters() order; `step` a 0-dim float32 CPU tensor
    def state_dict(self):
        self._warn_pending()
        steps = self.steps_taken()
        state = {}
        for i, (name, shape, off, numel, kind) in enumerate(self._params()):
            state[i] = {'step': torch.tensor(float(steps), dtype=torch.float32)}
            for key, flat in self._moments(self.param_groups[0]):
                state[i][key] = flat[off:off + numel].view(shape).clone()
        return {'state': state, 'param_groups': self._state_groups()}

    def load_state_dict(self, sd):
        """Accepts this class's own files and torch.optim.Adam's / AdamW's: `state` is keyed by the entries of param_groups[0]['params']
        (positions or arbitrary ids), in parameters() order.  The moments are replaced: an entry that is missing or has another size is
        reported and left at zero.  `step` goes back to the device (pa_adam_set_steps).  The file of another optimizer (RMSprop's:
        square_avg and no exp_avg) loads with ONE warning that says so and leaves this optimizer's options, zero moments and step 0."""
        import warnings
        params = self._params()
        state = sd.get('state', {})
        file_group = sd['param_groups'][0]
        entries = [st for st in state.values() if isinstance(st, dict)]
        if entries and not any('exp_avg' in st for st in entries):
            other = sorted(set(k for st in entries for k in st) - set(['step']))
            warnings.warn('optimizer state holds %s and no exp_avg: not an Adam file (another optimizer wrote it); the moments start at '
                          'zero, step 0, and this optimizer keeps its own options' % (', '.join(other) or 'no moments'))
            for _, flat in self._moments(self.param_groups[0]):
                flat.zero_()
            self._set_steps(0)
            return
        group = dict(self.param_groups[0])
        group.update((k, v) for k, v in file_group.items() if k in _ADAM_KEYS)
        group['betas'] = tuple(group['betas'])
        moments = self._moments(group)
        for _, flat in moments:
            flat.zero_()
        loaded = dict((key, 0) for key, _ in moments)
        keys, matched = self._file_keys(sd)
        if keys is None:
            warnings.warn('optimizer state has %d parameters, the network %d: the moments are not loaded'
                          % (sum(len(fg.get('params', [])) for fg in sd['param_groups']), len(params)))
            keys = []
        steps = set()
        frozen = self._frozen_params()
        for i, (key, (name, shape, off, numel, kind)) in enumerate(zip(keys, params)):
            st = state.get(key)
            if st is None:
                if i in frozen:                         # (torch keeps no state for a parameter it never stepped)
                    for mkey in loaded:
                        loaded[mkey] += 1
                continue
            for mkey, flat in moments:
                e = st.get(mkey)
                if e is None:
                    continue
                e = torch.as_tensor(e)
                if e.numel() != numel:
                    warnings.warn('optimizer state of %s: %s has %d elements, expected %d: skipped' % (name, mkey, e.numel(), numel))
                    continue
                flat[off:off + numel] = e.reshape(-1).to(flat.device, torch.float32)
                loaded[mkey] += 1
            if 'step' in st:
                steps.add(int(float(st['step'])))
        if state and keys:
            for mkey, _ in moments:
                if loaded[mkey] < len(params):
                    warnings.warn('optimizer state: %d of %d parameters had no %s entry (left at zero)' % (len(params) - loaded[mkey], len(params), mkey))
        if len(steps) > 1:
            warnings.warn('optimizer state: the parameters have different step counts %s; the largest is used' % sorted(steps))
        self._set_steps(max(steps) if steps else 0)
        if not self._grouped() and len(sd['param_groups']) == 1:
            self.param_groups[0].update(group)
        else:
            self._load_groups(sd, matched, tuple(k for k in _ADAM_KEYS if k not in ('lr', 'weight_decay')))

    def _set_steps(self, steps):
        check(lib().pa_adam_set_steps(ptr(self._state), int(steps), stream()), 'pa_adam_set_steps')


class AdamW(Adam):
    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, max_grad_norm=None, overlap=False, groups=None):
        """torch.optim.AdamW: Adam with decoupled weight decay and torch's default weight_decay"""
        Adam.__init__(self, net, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, decoupled_weight_decay=True,
                      max_grad_norm=max_grad_norm, overlap=overlap, groups=groups)


_SGD_KEYS = ('lr', 'momentum', 'weight_decay', 'nesterov', 'trust_coefficient', 'lars_eps', 'always_adapt')
# what torch.optim.SGD's step reads from a loaded param group beside this class's keys
_TORCH_SGD_EXTRA = {'dampening': 0, 'maximize': False, 'foreach': None, 'differentiable': False, 'fused': None}


class SGD(_FlatOptimizer):
    def __init__(self, net, lr, momentum=0, weight_decay=0, nesterov=False, max_grad_norm=None, overlap=False, groups=None,
                 trust_coefficient=0.0, eps=1e-8, always_adapt=False):
        """torch.optim.SGD(momentum, weight_decay, nesterov, dampening=0) as ONE launch on the flat arrays (pa_lars_step with
        trust_coefficient 0): d = g + weight_decay p; buf = momentum buf + d; d = nesterov ? d + momentum buf : buf; p -= lr d.
        momentum, nesterov (and LARS's trust_coefficient, lars_eps, always_adapt) live in param_groups[0] and are read at every step;
        lr, weight_decay and frozen are per group.  max_grad_norm, overlap, groups, accumulate(): as for RMSprop.  momentum_buffer is
        allocated when momentum is first non-zero (zeros, which gives torch's first step buf = d)."""
        if not momentum >= 0 or not weight_decay >= 0 or not float(lr) >= 0:
            raise ValueError('lr, momentum and weight_decay must be >= 0')
        if nesterov and momentum == 0:
            raise ValueError('nesterov needs momentum > 0')
        if not trust_coefficient >= 0 or not eps >= 0:
            raise ValueError('trust_coefficient and eps must be >= 0')
        self._attach(net, max_grad_norm, overlap)
        self._init_groups({'lr': lr, 'momentum': momentum, 'weight_decay': weight_decay, 'nesterov': bool(nesterov),
                           'trust_coefficient': trust_coefficient, 'lars_eps': eps, 'always_adapt': bool(always_adapt)}, groups)
        self._init_segments()
        self.momentum_buffer = None
        self._ensure_state(self.param_groups[0])
        self._skip_state = torch.zeros(2, dtype=torch.int32, device=net.flat_params.device)
        self.steps = 0

    def _ensure_state(self, g):
        if g.get('momentum', 0) != 0 and self.momentum_buffer is None:
            self.momentum_buffer = torch.zeros_like(self.net.flat_params)

    def step(self):
        g = self.param_groups[0]
        gscale = self._exchanged_gscale()
        n = self.net.flat_params.numel()
        mom, tc = float(g.get('momentum', 0)), float(g.get('trust_coefficient', 0))
        if g.get('nesterov', False) and mom == 0:
            raise ValueError('nesterov needs momentum > 0')
        self._ensure_state(g)
        tab, ngroups, frozen = self._group_table()
        coef = self._clip_coef(n, gscale, frozen)
        o = _lib.LarsOpts(mom, tc, float(g.get('lars_eps', 0)), int(bool(g.get('nesterov', False))), int(bool(g.get('always_adapt', False))))
        trust = tc > 0
        check(lib().pa_lars_step(C.byref(o), tab, ngroups, ptr(self._segs), self._nsegs, self._ntensors, ptr(self.net.flat_params),
                                 ptr(self.net.flat_grads), ptr(self.momentum_buffer) if mom != 0 else None, n, float(gscale), coef,
                                 ptr(self._layer_ws) if trust else None, ptr(self._norms) if trust else None,
                                 ptr(self._trust) if trust else None, ptr(self._skip_state), stream()), 'pa_lars_step')
        self._trusted = trust
        self.steps += 1
        self._weights_stepped()

    skip_flag_ptr = RMSprop.skip_flag_ptr
    skipped_steps = RMSprop.skipped_steps

    # torch.optim.SGD's format: state[i] = {'momentum_buffer': tensor} in parameters() order, empty without momentum
    def state_dict(self):
        self._warn_pending()
        state = {}
        if self.param_groups[0].get('momentum', 0) != 0:
            self._ensure_state(self.param_groups[0])
            for i, (name, shape, off, numel, kind) in enumerate(self._params()):
                state[i] = {'momentum_buffer': self.momentum_buffer[off:off + numel].view(shape).clone()}
        groups = self._state_groups()
        for pg in groups:
            for k, v in _TORCH_SGD_EXTRA.items():
                pg.setdefault(k, v)
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, sd):
        """Accepts this class's own files and torch.optim.SGD's.  momentum_buffer is replaced: an entry that is missing or has another
        size is reported and left at zero.  The file of another optimizer (square_avg or exp_avg and no momentum_buffer) loads with ONE
        warning that says so and leaves this optimizer's options and a zero momentum buffer."""
        import warnings
        params = self._params()
        state = sd.get('state', {})
        entries = [st for st in state.values() if isinstance(st, dict) and st]
        if entries and not any('momentum_buffer' in st for st in entries):
            other = sorted(set(k for st in entries for k in st) - set(['step']))
            warnings.warn('optimizer state holds %s and no momentum_buffer: not an SGD file (another optimizer wrote it); the momentum '
                          'buffer starts at zero and this optimizer keeps its own options' % (', '.join(other) or 'no buffers'))
            if self.momentum_buffer is not None:
                self.momentum_buffer.zero_()
            return
        group = dict(self.param_groups[0])
        group.update((k, v) for k, v in sd['param_groups'][0].items() if k in _SGD_KEYS)
        self._ensure_state(group)
        if self.momentum_buffer is not None:
            self.momentum_buffer.zero_()
        keys, matched = self._file_keys(sd)
        if keys is None:
            warnings.warn('optimizer state has %d parameters, the network %d: momentum_buffer not loaded'
                          % (sum(len(fg.get('params', [])) for fg in sd['param_groups']), len(params)))
            keys = []
        loaded, frozen = 0, self._frozen_params()
        if group.get('momentum', 0) != 0:
            for i, (key, (name, shape, off, numel, kind)) in enumerate(zip(keys, params)):
                e = (state.get(key) or {}).get('momentum_buffer')
                if e is None:
                    loaded += i in frozen               # (torch keeps no state for a parameter it never stepped)
                    continue
                e = torch.as_tensor(e)
                if e.numel() != numel:
                    warnings.warn('optimizer state of %s: momentum_buffer has %d elements, expected %d: skipped' % (name, e.numel(), numel))
                    continue
                self.momentum_buffer[off:off + numel] = e.reshape(-1).to(self.momentum_buffer.device, torch.float32)
                loaded += 1
            if state and keys and loaded < len(params):
                warnings.warn('optimizer state: %d of %d parameters had no momentum_buffer entry (left at zero)' % (len(params) - loaded, len(params)))
        if not self._grouped() and len(sd['param_groups']) == 1:
            self.param_groups[0].update(group)
        else:
            self._load_groups(sd, matched, tuple(k for k in _SGD_KEYS if k not in ('lr', 'weight_decay')))


class LARS(SGD):
    def __init__(self, net, lr, momentum=0.9, weight_decay=0, nesterov=False, trust_coefficient=1e-3, eps=1e-8, always_adapt=False,
                 max_grad_norm=None, overlap=False, groups=None):
        """LARS (You, Gitman, Ginsburg 2017) on SGD with momentum: every tensor's d = g + weight_decay p is multiplied by
        r_t = trust_coefficient ||w|| / (||g|| + weight_decay ||w|| + eps) before the momentum, with the norms taken per tensor on the
        device (two more launches in front of the step; squares and sums in double, no atomics).  r_t = 1 for an all-zero tensor, a zero
        gradient and -- unless always_adapt -- a tensor whose group has no weight decay (BatchNorm and biases under --no_decay_1d).
        last_trust() / tensor_norms(): the ratios and norms of the last step, on the device, for logging."""
        SGD.__init__(self, net, lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov, max_grad_norm=max_grad_norm,
                     overlap=overlap, groups=groups, trust_coefficient=trust_coefficient, eps=eps, always_adapt=always_adapt)


_LAMB_KEYS = ('max_trust', 'always_adapt')


class LAMB(Adam):
    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, max_trust=0, always_adapt=False, max_grad_norm=None,
                 overlap=False, groups=None):
        """LAMB (You et al. 2020): Adam's moments, u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + weight_decay p, and per tensor
        p -= lr r_t u with r_t = ||w|| / ||u|| (1 where either norm is 0, and -- unless always_adapt, the default of apex FusedLAMB and
        timm -- for a tensor whose group has no weight decay), capped at max_trust when that is > 0.  pa_lamb_step: prologue, a pass
        that updates the moments and sums ||w||^2 and ||u||^2 per tensor, the ratios, a pass that applies the step.  The state is
        Adam's (exp_avg, exp_avg_sq, the step count on the device): state_dict() has Adam's keys, and a file goes both ways.  amsgrad is
        not supported.  last_trust() / tensor_norms(): as for LARS."""
        b1, b2 = betas
        if not (0 <= b1 < 1 and 0 <= b2 < 1):
            raise ValueError('betas must be in [0, 1)')
        if not eps > 0 or weight_decay < 0 or not max_trust >= 0:
            raise ValueError('eps must be > 0, weight_decay and max_trust >= 0')
        self._attach(net, max_grad_norm, overlap)
        self._init_groups({'lr': lr, 'betas': (b1, b2), 'eps': eps, 'weight_decay': weight_decay, 'amsgrad': False, 'max_trust': max_trust,
                           'always_adapt': bool(always_adapt)}, groups)
        self._init_segments()
        self.exp_avg = torch.zeros_like(net.flat_params)
        self.exp_avg_sq = torch.zeros_like(net.flat_params)
        self.max_exp_avg_sq = None
        self._state = torch.zeros(8, dtype=torch.int32, device=net.flat_params.device)

    def _ensure_state(self, g):
        if g.get('amsgrad', False):
            raise ValueError('LAMB: amsgrad is not supported')

    def step(self):
        g = self.param_groups[0]
        self._ensure_state(g)
        gscale = self._exchanged_gscale()
        n = self.net.flat_params.numel()
        b1, b2 = g['betas']
        tab, ngroups, frozen = self._group_table()
        coef = self._clip_coef(n, gscale, frozen)
        o = _lib.LambOpts(float(b1), float(b2), float(g['eps']), float(g.get('max_trust', 0)), int(bool(g.get('always_adapt', False))), 0)
        check(lib().pa_lamb_step(C.byref(o), tab, ngroups, ptr(self._segs), self._nsegs, self._ntensors, ptr(self.net.flat_params),
                                 ptr(self.net.flat_grads), ptr(self.exp_avg), ptr(self.exp_avg_sq), n, float(gscale), coef, ptr(self._layer_ws),
                                 ptr(self._norms), ptr(self._trust), ptr(self._state), stream()), 'pa_lamb_step')
        self._trusted = True
        self._weights_stepped()

    def load_state_dict(self, sd):
        """Adam.load_state_dict (an Adam / AdamW file loads: its moments and step count; max_exp_avg_sq and the decay mode are not
        LAMB's and are dropped); max_trust and always_adapt come from a LAMB file's group 0."""
        fgs = [dict((k, v) for k, v in fg.items() if k != 'decoupled_weight_decay') for fg in sd['param_groups']]
        for fg in fgs:
            fg['amsgrad'] = False
        Adam.load_state_dict(self, dict(sd, param_groups=fgs))
        for g in self.param_groups:
            g.pop('decoupled_weight_decay', None)
            g.update((k, fgs[0][k]) for k in _LAMB_KEYS if k in fgs[0])


class ModelEma(object):
    def __init__(self, net, decay=0.999, warmup=False, buffers='ema'):
        """Exponential moving average of the weights of `net` (any _HipModule: the pose net or an agent), kept on the device:
        ema += (1 - decay) (p - ema) after every optimizer step that was TAKEN (pa_ema_advance + pa_ema_lerp, fp32 like torch's
        swa_utils.get_ema_multi_avg_fn).  self.module is a twin of `net` -- the same class and configuration, its own flat arrays and
        handles -- that holds the average and is a normal net: eval(), forward, heatmaps, accuracy, pckh_origin_res, state_dict().
        warmup: decay_t = min(decay, (1 + t) / (10 + t)) with t = updates so far, so that the first steps do not average against the
        initial weights for 1 / (1 - decay) steps.  buffers: 'ema' averages the BatchNorm running statistics like the parameters,
        'copy' takes the net's own.
        The update count, the count of held steps and the weight of the step live on the device (self._state, a pa_ema_state): the fp16
        build decides there whether the optimizer's step is taken, and update(optimizer) reads that optimizer's flag there, so the
        average does not move, and the warm-up count does not advance, on a skipped step.  updates() / held() read them (synchronising).
        Several GPUs: every rank holds the same parameters after the step (the gradient is summed before it), so every rank forms the
        same average without any exchange; the BatchNorm statistics are per rank, in the average as in the net.
        Create it after the checkpoint load and broadcast_parameters, or call reset() after them.
        The average is fp32: at decay 0.9999 an increment (1 - decay) (p - ema) below half an ulp of the average is lost."""
        if not 0 <= float(decay) < 1:
            raise ValueError('decay must be in [0, 1)')
        if buffers not in ('ema', 'copy'):
            raise ValueError("buffers must be 'ema' or 'copy'")
        self.net, self.decay, self.warmup, self.buffers = net, float(decay), bool(warmup), buffers
        net._ensure_table()
        self.module = net._twin()
        self.module._ensure_table()
        self.module.eval()
        self._state = torch.zeros(8, dtype=torch.int32, device=net.flat_params.device)
        self.reset()

    def reset(self):
        """the twin becomes a bit-exact copy of the net again (parameters, buffers, num_batches_tracked) and the counts go to 0"""
        m = self.module
        m.flat_params.copy_(self.net.flat_params)
        m.flat_buffers.copy_(self.net.flat_buffers)
        m._nbt = self.net._nbt
        self._state.zero_()
        m.weights_changed()

    def update(self, optimizer=None):
        """Call after optimizer.step(), on the same stream: one prologue that reads the optimizer's skip flag (None: every call
        averages), one launch over the parameters, one over the buffers.  The twin's 16-bit weight copies are re-packed at its next
        use, not here."""
        m, net = self.module, self.net
        flag = optimizer.skip_flag_ptr() if optimizer is not None else None
        check(lib().pa_ema_advance(ptr(self._state), self.decay, int(self.warmup), flag, stream()), 'pa_ema_advance')
        check(lib().pa_ema_lerp(ptr(m.flat_params), ptr(net.flat_params), net.flat_params.numel(), ptr(self._state), 0, stream()), 'pa_ema_lerp')
        check(lib().pa_ema_lerp(ptr(m.flat_buffers), ptr(net.flat_buffers), net.flat_buffers.numel(), ptr(self._state),
                                1 if self.buffers == 'copy' else 0, stream()), 'pa_ema_lerp')
        m._nbt = net._nbt
        m.weights_changed()

    def _counts(self):
        updates, held = C.c_longlong(0), C.c_longlong(0)
        check(lib().pa_ema_counts(ptr(self._state), C.byref(updates), C.byref(held), stream()), 'pa_ema_counts')
        return int(updates.value), int(held.value)

    def updates(self):
        """averaging steps applied so far, read from the device: synchronises the stream"""
        return self._counts()[0]

    def held(self):
        """update() calls that left the average where it was because the optimizer had skipped its step (fp16 build)"""
        return self._counts()[1]

    def state_dict(self):
        return {'decay': self.decay, 'warmup': self.warmup, 'buffers': self.buffers, 'updates': self.updates(), 'module': self.module.state_dict()}

    def load_state_dict(self, sd):
        """the options, the averaged weights and the update count (back on the device: pa_ema_set_updates) of state_dict()"""
        decay, buffers = float(sd['decay']), sd['buffers']
        if not 0 <= decay < 1 or buffers not in ('ema', 'copy'):
            raise ValueError('ModelEma.load_state_dict: decay %r / buffers %r' % (sd['decay'], buffers))
        self.decay, self.warmup, self.buffers = decay, bool(sd['warmup']), buffers
        self.module.load_state_dict(sd['module'])
        self._state.zero_()
        check(lib().pa_ema_set_updates(ptr(self._state), int(sd['updates']), stream()), 'pa_ema_set_updates')


def make_ema(opt, net):
    """The weight average the command line asks for (options/train_options.py: --ema_decay D --ema_warmup 0|1 --ema_buffers ema|copy);
    None with --ema_decay 0, the default: no twin, no launch."""
    decay = float(getattr(opt, 'ema_decay', 0) or 0)
    if decay == 0:
        return None
    return ModelEma(net, decay=decay, warmup=bool(getattr(opt, 'ema_warmup', 0)), buffers=getattr(opt, 'ema_buffers', 'ema'))


def accum_plan(n_batches, accum_steps):
    """--accum_steps N over an epoch of n_batches iterations: per iteration (steps, group size so far).  Iteration i ends its group with
    an optimizer step when i % N == N - 1 or i is the last of the epoch (a short trailing group is stepped with its real size, so an
    epoch never ends with a gradient pending); every other iteration calls accumulate().  The sizes at the stepping iterations sum to
    n_batches.  Pure host logic."""
    n, N = int(n_batches), int(accum_steps)
    if N < 1:
        raise ValueError('accum_steps must be >= 1')
    return [(i % N == N - 1 or i == n - 1, i % N + 1) for i in range(n)]


def make_optimizer(opt, net, lr, overlap=False):
    """The optimizer the command line asks for (options/train_options.py: --optimizer rmsprop | adam | adamw | sgd | lars | lamb).  rmsprop, the default:
    the reference's recipe (alpha 0.99, eps 1e-8) with optim_options(opt).  adam / adamw: --beta1 --beta2 --adam_eps --amsgrad;
    --weight_decay (coupled for adam, decoupled for adamw; passed as given, so 0 means none for adamw too) and --clip_grad_norm are
    shared between the kinds.  sgd / lars: --momentum (sgd: required > 0) --nesterov (lars: --trust_coef --always_adapt); lamb: --beta1 --beta2 --adam_eps
    --max_trust --always_adapt; --centered, --amsgrad and --nesterov without momentum are refused with them."""
    kind = getattr(opt, 'optimizer', 'rmsprop')
    groups = group_specs(opt, net)
    if kind == 'rmsprop':
        return RMSprop(net, lr=lr, alpha=0.99, eps=1e-8, overlap=overlap, groups=groups, **optim_options(opt))
    clip = float(getattr(opt, 'clip_grad_norm', 0) or 0)
    if kind in ('sgd', 'lars', 'lamb'):
        mom, nesterov = float(getattr(opt, 'momentum', 0) or 0), bool(getattr(opt, 'nesterov', 0))
        if getattr(opt, 'centered', 0) or getattr(opt, 'amsgrad', 0):
            raise ValueError('--centered and --amsgrad are RMSprop / Adam options: not with --optimizer %s' % kind)
        if kind == 'sgd' and mom == 0:
            raise ValueError('--optimizer sgd needs --momentum > 0 (gradient descent without momentum: utils.optim.SGD(net, lr) in code)')
        if nesterov and (kind == 'lamb' or mom == 0):
            raise ValueError('--nesterov needs --optimizer sgd or lars and --momentum > 0')
        kw = dict(lr=lr, weight_decay=float(getattr(opt, 'weight_decay', 0) or 0), max_grad_norm=clip if clip > 0 else None, overlap=overlap,
                  groups=groups)
        always = bool(getattr(opt, 'always_adapt', 0))
        if kind == 'lamb':
            if mom != 0:
                raise ValueError('--momentum is an RMSprop / SGD option: not with --optimizer lamb')
            return LAMB(net, betas=(float(getattr(opt, 'beta1', 0.9)), float(getattr(opt, 'beta2', 0.999))), eps=float(getattr(opt, 'adam_eps', 1e-8)),
                        max_trust=float(getattr(opt, 'max_trust', 0) or 0), always_adapt=always, **kw)
        if kind == 'lars':
            return LARS(net, momentum=mom, nesterov=nesterov, trust_coefficient=float(getattr(opt, 'trust_coef', 1e-3)), always_adapt=always, **kw)
        return SGD(net, momentum=mom, nesterov=nesterov, **kw)
    if kind not in ('adam', 'adamw'):
        raise ValueError('unknown optimizer %r' % (kind,))
    if float(getattr(opt, 'momentum', 0) or 0) != 0 or getattr(opt, 'centered', 0):
        raise ValueError('--momentum and --centered are RMSprop options: not with --optimizer %s' % kind)
    clip = float(getattr(opt, 'clip_grad_norm', 0) or 0)
    kw = dict(lr=lr, betas=(float(getattr(opt, 'beta1', 0.9)), float(getattr(opt, 'beta2', 0.999))), eps=float(getattr(opt, 'adam_eps', 1e-8)),
              weight_decay=float(getattr(opt, 'weight_decay', 0) or 0), amsgrad=bool(getattr(opt, 'amsgrad', 0)),
              max_grad_norm=clip if clip > 0 else None, overlap=overlap, groups=groups)
    return (AdamW if kind == 'adamw' else Adam)(net, **kw)


def group_specs(opt, net):
    """The `groups` argument the command line asks for (options/train_options.py: --no_decay_1d 1, --freeze REGEX, --lr_group REGEX:MULT,
    repeatable); None with all of them off, the default: one group.  --freeze and --lr_group are the pose net's (a net with
    num_stacks); the agent's optimizer takes --no_decay_1d only.  Order, first match wins: the frozen tensors, then every --lr_group
    in the order given, then the remaining 1-D tensors.  With --no_decay_1d the 1-D tensors of an --lr_group form a group of their own
    (that rate, no decay).  A REGEX that matches no parameter is an error, so a typo cannot silently train everything."""
    import re
    no_decay = bool(getattr(opt, 'no_decay_1d', 0))
    pose = hasattr(net, 'num_stacks')
    freeze = (getattr(opt, 'freeze', '') or '') if pose else ''
    lr_groups = list(getattr(opt, 'lr_group', None) or []) if pose else []
    if not (no_decay or freeze or lr_groups):
        return None
    net._ensure_table()
    params = [(t[0], tuple(t[1])) for t in net._table if t[4] == 0]
    left = list(params)
    specs = []

    def take(what, rx, **values):
        hit = [(n, s) for n, s in left if re.search(rx, n)]
        if not [1 for n, s in params if re.search(rx, n)]:
            raise ValueError('%s %r matches no parameter of the net' % (what, rx))
        split = no_decay and 'frozen' not in values          # the 1-D tensors of the match: a group of their own, without decay
        one_d = [t for t in hit if len(t[1]) <= 1] if split else []
        for part, v in ((one_d, dict(values, weight_decay=0.0)), ([t for t in hit if t not in one_d], values)):
            if part:
                specs.append(dict(v, params=[n for n, _ in part]))
        left[:] = [t for t in left if t not in hit]

    if freeze:
        take('--freeze', freeze, frozen=True)
    for item in lr_groups:
        rx, sep, mult = item.rpartition(':')
        try:
            mult = float(mult)
        except ValueError:
            sep = ''
        if not sep or not rx or not mult >= 0:
            raise ValueError('--lr_group %r: expected REGEX:MULT with MULT >= 0' % (item,))
        take('--lr_group', rx, lr_mult=mult)
    if no_decay:
        rest = [n for n, s in left if len(s) <= 1]
        if rest:
            specs.append(dict(params=rest, weight_decay=0.0))
    return specs
