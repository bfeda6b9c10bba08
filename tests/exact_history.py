"""The step the exact checks look at, and what came before it.

tests/bn_exact.py, tests/conv_exact.py and tests/asn_exact.py recompute every tensor of ONE step in float64.  On the first step after
pa_net_bind a whole class of defects cannot show: the engine relies on state that the bind establishes (a zero-filled workspace: the
per-stack loss accumulators, the padding channels of the 16-channel head tensors, the statistic accumulators) and that from then on
only the kernels themselves keep right (loss_out_kernel clears the accumulators at the end of a forward pass; the weight copies in the
storage type are repacked after every optimizer step; pa_launch_bn_eval writes eval-mode constants into the tables the training
finalize fills).  A residue in any of these gives a step that is right the first time and wrong from the second on.  The drivers
therefore take a `history` that is run in front of the checked step; this module brings net, optimizer and inputs into that history,
snapshots the parameters and running estimates IMMEDIATELY before the checked step, runs it and hands back what the drivers use.

'fresh' is the step the legs have always checked: seeded NCHW fp32 images (tests/inputs.py), no step before it.  Every other history
runs the checked step as bench.py runs its timed steps (stack_hg.train_step): DeviceBatch.synthetic + Augmenter -> img4 (NHWC4 in the
storage type; the image the checks use is its first three channels as NCHW), loss_and_backward(img4=..., pts=..., after_forward=
the two meters of train_step), two batches in alternation so that no step sees the input of the step before:
  warm        three train_step calls (RMSprop, lr 2.5e-4), then the checked step: accumulator residue, repacked weights (Checker.W
              rounds the CURRENT fp32 parameters), running estimates from a non-initial state;
  graph       net.use_graph = True: capture, two replays, the checked step is the fourth launch of the graph (no after_forward: the
              two passes are one launch), the debug views are read after a replay;
  phased      RMSprop(net, overlap=True) in a single process: the backward pass goes through pa_hg_backward_phase; two steps, then
              the checked step;
  after_eval  one train_step; an eval-mode forward of the other batch; a train-mode forward of it with no loss and no backward (a
              forward that never reached loss_out, in the NCHW fp32 entry); the checked step: eval constants left in the BatchNorm
              tables, the heat-peak cache, the training statistics of a forward nobody finished;
  after_half  one train_step; the agent's half-hourglass forward on the pose net in train mode (pa_hg_forward_half, train = 1) and an
              agent backward with seeded targets; the checked FULL step.  The agent needs res >= 256.
  after_masked  one loss_and_backward(dropout_masks=...) and an optimizer step, then the checked step WITHOUT masks: what a masked step
              leaves behind (Net::drop_mask, Hourglass::low_done / Residual::low_of_in, the gradients of the masked copies) while the
              fused upsample-add paths and the consumer-prologue finalizes come back on.  The mask needs a 4 x 4 neck: res 256.
masks (a seed): the checked step is the occlusion agent's training step, loss_and_backward(dropout_masks=M), M [B][1][4][4] of 0 / 1 with
two zero cells per sample (drop_masks); the steps of 'warm' in front of it are masked too, each with another draw (loss_and_backward
and the optimizer called as train_step calls them: train_step takes no masks).  Only with 'fresh' and 'warm': a captured graph and the
phased backward pass do not run with masks.
For the agent (agent_history): 'warm' is two pose train_step calls and two agent steps (forward, backward or backward_masks,
an RMSprop step of the agent's own optimizer); 'after_eval' one agent step and the same eval / train-forward interleaving on the
agent.  Before the agent steps the pose net's running estimates are set to the statistics of a crop batch (calibrate)."""
import numpy as np
import torch

POSE_HISTORIES = ('fresh', 'warm', 'graph', 'phased', 'after_eval', 'after_half', 'after_masked')
AGENT_HISTORIES = ('fresh', 'warm', 'after_eval')
LR = 2.5e-4


class Feed(object):
    """two synthetic batches in alternation through one Augmenter (the benchmark's input path)"""
    def __init__(self, B, res, seed):
        from pose_adv_aug_amd.data import Augmenter, DeviceBatch
        self.batches = [DeviceBatch.synthetic(B, seed=1000 * seed + k) for k in (0, 1)]
        self.aug = Augmenter(seed=seed, inp_res=res, out_res=res // 4)
        self.k = 0

    def next_batch(self):
        b = self.batches[self.k % 2]
        self.k += 1
        return b

    def next_data(self, want_nchw=False):
        return self.aug.regular(self.next_batch(), want_nchw=want_nchw)


def _meters(net, data):
    from pose_adv_aug_amd.stack_hg import PCK_IDX

    def meters():           # the two meters of stack_hg.train_step
        pckh = net.accuracy(PCK_IDX)
        pckh_o, _ = net.pckh_origin_res(data['c'], data['s'], data['r'], data['grnd_pts'], data['normalizer'])
        return pckh, pckh_o
    return meters


def img_of(img4):
    """the image as the engine read it: the first three channels of NHWC4, as NCHW fp32 (exact: storage-type values)"""
    return img4[..., :3].permute(0, 3, 1, 2).float().contiguous()


def _snapshot(module):
    sd0 = {k: v.clone() for k, v in module.state_dict().items()}
    before = {k: v for k, v in sd0.items() if k.endswith('running_mean') or k.endswith('running_var')}
    return sd0, before


class Step(object):
    """the checked pose step: net; sd0 / before (all entries / the running estimates, cloned immediately before it); img (NCHW fp32, as
    the engine read it); pts (device) and pts_np; grads, outs, loss_total and losses (the per-stack values) after it; masks: the
    [B][1][4][4] occlusion masks of the checked step (device, fp32) or None"""


FORCED_CELLS = ((0, 15), (5, 6))        # sample 0: two corners of the map; sample 1: interior and adjacent


def drop_masks(seed, B, draw=0):
    """[B][1][4][4] fp32 of 0 / 1, two distinct zero cells per sample (what pa_sample_dropout_masks draws).  Draw 0, the checked step's:
    samples 0 and 1 take FORCED_CELLS, so that every leg has cells on the map border and a pair sharing an edge."""
    from tests import inputs
    g = inputs.rng(seed, 77, draw)
    M = torch.ones(B, 1, 4, 4)
    for b in range(B):
        cells = g.choice(16, 2, replace=False)
        if draw == 0 and b < len(FORCED_CELLS):
            cells = FORCED_CELLS[b]
        for cell in cells:
            M[b, 0, int(cell) // 4, int(cell) % 4] = 0
    assert bool((M.view(B, 16).sum(1) == 14).all())
    return M


def _masked_train_step(net, opt, data, M):
    """stack_hg.train_step with masks: the same two calls"""
    net.loss_and_backward(img4=data['img4'], pts=data['pts'], dropout_masks=M, after_forward=_meters(net, data))
    opt.step()


def pose_step(stacks, chan, B, res, seed, history='fresh', masks=None):
    from pose_adv_aug_amd.stack_hg import train_step
    from pose_adv_aug_amd.utils.optim import RMSprop
    from tests import inputs
    from tests.test_gpu_net import t, _hg_pair
    assert history in POSE_HISTORIES, history
    assert masks is None or history in ('fresh', 'warm'), 'no masked step behind %s' % history
    torch.cuda.set_device(0)
    ref, net = _hg_pair(stacks, chan, B, res, seed=seed)
    del ref
    S = Step()
    S.net, S.history = net, history
    S.masks = None if masks is None else drop_masks(masks, B).cuda()
    net.train()
    if history == 'fresh':
        S.sd0, S.before = _snapshot(net)
        S.img = t(inputs.images(seed + 100, B, res)).cuda()
        S.pts_np = inputs.heat_pts(seed + 101, B, res=res // 4)
        S.pts = t(S.pts_np).cuda()
        loss, S.outs = net.loss_and_backward(S.img, S.pts, want_outputs=True, dropout_masks=S.masks)
    else:
        feed = Feed(B, res, seed)
        opt = RMSprop(net, lr=LR, overlap=(history == 'phased'))
        if history == 'graph':
            net.use_graph = True
        for k in range({'warm': 3, 'graph': 3, 'phased': 2, 'after_eval': 1, 'after_half': 1, 'after_masked': 0}[history]):
            if masks is None:
                train_step(net, opt, feed.aug, feed.next_batch())
            else:
                _masked_train_step(net, opt, feed.next_data(), drop_masks(masks, B, draw=k + 1).cuda())
        if history == 'after_masked':
            _masked_train_step(net, opt, feed.next_data(), drop_masks(seed, B).cuda())
        if history == 'after_eval':
            other = feed.next_data(want_nchw=True)
            net.eval()
            net(img4=other['img4'])
            net.train()
            net(other['img'])
        if history == 'after_half':
            from pose_adv_aug_amd.models.asn_stacked_hg import create_asn
            from tests.asn_exact import _targets
            agent = create_asn(chan, chan, 7, 7, is_aug=True, res=res, default_batch=B)
            agent.reset_parameters(seed=seed + 1)
            agent.train()
            other = feed.next_data()
            ls, lr = net(asn=agent, is_half_hg=True, is_aug=True, img4=other['img4'])
            gs_t, gr_t = _targets(seed + 2, ls, lr, B)
            agent.loss_and_backward(gs_t, gr_t)
            S.agent = agent         # (alive until the checks are done)
        data = feed.next_data()          # (no zero_grad: the loops never call it, the backward pass overwrites flat_grads)
        torch.cuda.synchronize()
        S.sd0, S.before = _snapshot(net)
        S.img, S.pts = img_of(data['img4']), data['pts']
        S.pts_np = S.pts.cpu().numpy().astype(np.float64)
        if history == 'graph':
            loss, S.outs = net.loss_and_backward(img4=data['img4'], pts=data['pts'], want_outputs=True)
        else:
            loss, S.outs = net.loss_and_backward(img4=data['img4'], pts=data['pts'], want_outputs=True, dropout_masks=S.masks,
                                                 after_forward=_meters(net, data))
        S.data = data
    S.loss_total = loss.clone()
    S.losses = net._last_losses
    torch.cuda.synchronize()
    S.grads = {n: g.clone() for n, g in net.named_grads()}
    return S


# ---------------------------------------------------------------------------------------------------------------------------------
def calibrate(net, img4):
    """Set the pose net's running BatchNorm estimates to the batch statistics of img4, as a trained net's are of its data (what
    asn_exact.oracle_pair does for the seeded images of the 'fresh' legs): the agent's legs run the pose net in eval mode, and with
    estimates from other data -- the seeded noise images, or weights two optimizer steps old -- its features drift until bn1 of the
    agent's input blocks sees |mean| / sigma in the hundreds and every bound there is degenerate (tests/asn_exact.py).  The engine's
    momentum is fixed, so one train-mode forward (no loss, no backward) is inverted: new = (1 - m) old + m batch in fp32."""
    from tests.bn_exact import MOM32, ONE_MINUS_MOM32
    m, om = float(np.float32(MOM32[0])), float(np.float32(1.0) - np.float32(MOM32[0]))
    assert abs(om - ONE_MINUS_MOM32[0]) < 1e-7
    was = net.training
    net.train()
    old = {k: v.double().clone() for k, v in net.state_dict().items() if k.endswith('running_mean') or k.endswith('running_var')}
    net(img4=img4)
    torch.cuda.synchronize()
    sd = net.state_dict()
    for k, o in old.items():
        b = (sd[k].double() - om * o) / m
        sd[k].copy_((b.clamp_min(0) if k.endswith('running_var') else b).float())
    net.train(was)


def agent_history(net, agent, B, res, seed, history, forward, backward):
    """Bring the pose net and the agent of an agent leg into `history` and return the forward of the checked step.
    forward(**image) runs the leg's half-hourglass + agent forward (image: x= or img4=) and returns what backward(out, k) needs;
    backward(out, k) zeroes the gradients and runs the leg's backward with seeded targets / gradients (k: a step counter for the seed).
    'fresh': the seeded NCHW image of the legs, no step before."""
    from pose_adv_aug_amd.stack_hg import train_step
    from pose_adv_aug_amd.utils.optim import RMSprop
    from tests import inputs
    from tests.test_gpu_net import t
    assert history in AGENT_HISTORIES, history
    if history == 'fresh':
        img = t(inputs.images(seed + 100, B, res)).cuda()
        net.eval(); agent.train()
        return lambda: forward(x=img)
    feed = Feed(B, res, seed)
    aopt = RMSprop(agent, lr=LR)
    if history == 'warm':
        popt = RMSprop(net, lr=LR)
        net.train()
        for _ in range(2):
            train_step(net, popt, feed.aug, feed.next_batch())
    calibrate(net, feed.next_data()['img4'])
    net.eval(); agent.train()
    for k in range(2 if history == 'warm' else 1):
        out = forward(img4=feed.next_data()['img4'])
        backward(out, k)
        aopt.step()
    if history == 'after_eval':
        other = feed.next_data()
        agent.eval()
        forward(img4=other['img4'])
        agent.train()
        forward(img4=other['img4'])
    data = feed.next_data()
    torch.cuda.synchronize()
    return lambda: forward(img4=data['img4'])
