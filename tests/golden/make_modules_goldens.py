#!/usr/bin/env python3
"""Generate tests/golden/hg_s1m2c128.npz by running THE REFERENCE's own create_hg(1, 2, 16, 128) -- two residual blocks per
hourglass site and in post_res (models/asn_stacked_hg.py:73-77, :272-276) -- through one training step, exactly as
make_goldens.py:gen_nets records hg_s1c128 for one block per site.
Run from the repo root:  python tests/golden/make_modules_goldens.py

The transliteration of the reference and the import are make_goldens.py's.  Only arrays are written: the train-mode heat maps,
the loss, the parameter count, the output layers' gradients in full (out_conv.0.*, linear.0.1.*), a digest of every gradient and
the eval-mode heat maps after one RMSprop step."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import OUT, digest, load_ref, t  # noqa: E402

STACKS, MODULES, CHAN, SEED = 1, 2, 128, 72


def gen_modules(R):
    from tests import inputs
    from oracle.model import deterministic_fill_
    M = R['M']
    torch.set_num_threads(8)
    net = M.create_hg(num_stacks=STACKS, num_modules=MODULES, num_classes=16, chan=CHAN)
    deterministic_fill_(net, seed=SEED)
    net.train()
    img = t(inputs.images(SEED + 100, 2, 128))
    pts = inputs.heat_pts(SEED + 200, 2, res=32)
    heat = t(inputs.heatmaps_from_pts(pts, res=32))
    assert np.array_equal(heat.numpy(), np.stack(
        [R['HumanPts'].pts2heatmap(pts[i].copy(), [32, 32])[0] for i in range(2)]).astype(np.float32))
    opt = torch.optim.RMSprop(net.parameters(), lr=2.5e-4, alpha=0.99, eps=1e-8, momentum=0, weight_decay=0)
    out = net(img)
    loss = 0
    for o in out:
        d = (o - heat) ** 2
        loss = loss + d.sum() / d.numel()
    opt.zero_grad()
    loss.backward()
    names = [n for n, _ in net.named_parameters()]
    grads = [p.grad.clone() for p in net.parameters()]
    opt.step()
    head = [n for n in names if n.startswith('out_conv.0.') or n.startswith('linear.0.1.')]
    rec = dict(out=np.stack([o.detach().numpy() for o in out]), loss=np.array(float(loss)),
               nparams=np.array(sum(p.numel() for p in net.parameters())), nkeys=np.array(len(net.state_dict())),
               head_names=np.array(head),
               head_grads=np.concatenate([g.flatten().numpy() for n, g in zip(names, grads) if n in head]),
               grad_digest=digest(grads))
    net.eval()
    with torch.no_grad():
        rec['out_eval'] = np.stack([o.numpy() for o in net(img)])
    path = os.path.join(OUT, 'hg_s%dm%dc%d.npz' % (STACKS, MODULES, CHAN))
    np.savez_compressed(path, **rec)
    print(os.path.basename(path), int(rec['nparams']), 'params, loss', float(loss), os.path.getsize(path) // 1024, 'KB')


if __name__ == '__main__':
    gen_modules(load_ref())
