"""Pins the float64 restatement of tests/seq_exact_checks.py (the reference of tests/test_emu_seq_exact.py and
tests/test_gpu_seq_exact.py) on the CPU: against torch.autograd in float64 over a direct torch transcription of PoolNet's
formulas written here (1e-12, every input family), against the live reference's own PoolNet in float64 where it is importable
(skipped where the golden-recipe tests skip), and against PoolNetOracle at its usual 1e-5 as a sanity check of the comparison."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seq_exact_checks as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE = os.path.isfile('/root/reference/spotlight/__init__.py')
RTOL = 1e-12

CASES = {
    'isolating-64-17-pointwise': lambda: sx.isolating_case(64, 17, 'pointwise', 5),
    'isolating-64-17-bpr': lambda: sx.isolating_case(64, 17, 'bpr', 5),
    'isolating-64-17-hinge': lambda: sx.isolating_case(64, 17, 'hinge', 5),
    'isolating-64-17-adaptive-5': lambda: sx.isolating_case(64, 17, 'adaptive_hinge', 5),
    'isolating-64-17-adaptive-1': lambda: sx.isolating_case(64, 17, 'adaptive_hinge', 1),
    'isolating-64-17-adaptive-4': lambda: sx.isolating_case(64, 17, 'adaptive_hinge', 4),
    'isolating-6-33-bpr': lambda: sx.isolating_case(6, 33, 'bpr', 1, B=3),
    'isolating-4-257-adaptive-5': lambda: sx.isolating_case(4, 257, 'adaptive_hinge', 5, B=3),
    'isolating-256-65-bpr': lambda: sx.isolating_case(256, 65, 'bpr', 1, B=3),
    'grid-stride-bpr': lambda: sx.isolating_case(8, 3, 'bpr', 1, B=35),
    'grid-stride-adaptive-5': lambda: sx.isolating_case(8, 3, 'adaptive_hinge', 5, B=35),
    'shared-64-64-bpr': lambda: sx.shared_case('bpr'),
    'shared-64-64-pointwise': lambda: sx.shared_case('pointwise'),
    'shared-64-17-hinge': lambda: sx.shared_case('hinge', 5, L=17),
    'shared-64-17-adaptive-5': lambda: sx.shared_case('adaptive_hinge', 5, L=17),
    'padding-64-17-bpr': lambda: sx.padding_case(64, 17, 'bpr', 1, 0),
    'padding-64-17-adaptive-5': lambda: sx.padding_case(64, 17, 'adaptive_hinge', 5, 0),
    'padding-6-33-bpr': lambda: sx.padding_case(6, 33, 'bpr', 1, 0),
    'padding-6-33-adaptive-5': lambda: sx.padding_case(6, 33, 'adaptive_hinge', 5, 0),
    'padding-64-17-bpr-bloom': lambda: sx.padding_case(64, 17, 'bpr', 1, 2),
    'padding-64-17-adaptive-5-bloom': lambda: sx.padding_case(64, 17, 'adaptive_hinge', 5, 2),
    'padding-6-33-bpr-bloom': lambda: sx.padding_case(6, 33, 'bpr', 1, 2),
    'padding-6-33-adaptive-5-bloom': lambda: sx.padding_case(6, 33, 'adaptive_hinge', 5, 2),
    'tie': lambda: sx.tie_case(),
}


def torch_minibatch(case):
    """PoolNet.user_representation + forward + the masked loss (sequence/representations.py:76-144, losses.py) transcribed into
    torch, float64; autograd does the backward.  Returns (loss, rep [B, L, D], final rep [B, D], dL/dE, dL/dbias)."""
    E = torch.tensor(case.E.astype(np.float64), requires_grad=True)
    b = torch.tensor(case.bias.astype(np.float64).reshape(-1, 1), requires_grad=True)
    seqs = torch.from_numpy(case.seqs)
    B, L = case.seqs.shape
    D = case.D
    nn = case.n_neg if case.loss == 'adaptive_hinge' else 1
    cand = torch.from_numpy(case.negs.reshape(nn, B, L))

    def vectors(ids):  # the item embedding layer: a ScaledEmbedding with padding_idx 0, or a BloomEmbedding over one
        if case.bloom is None:
            return F.embedding(ids, E, padding_idx=0)
        idx = torch.from_numpy(sx.hashed_rows(ids.numpy(), case.bloom, E.shape[0]))
        return F.embedding(idx, E, padding_idx=0).sum(1).view(ids.shape + (D,))

    x = F.pad(vectors(seqs).permute(0, 2, 1).unsqueeze(3), (0, 0, 1, 0))
    rep = (torch.cumsum(x, 2) / (torch.cumsum((x != 0.0).double(), 2) + 1)).squeeze(3)  # [B, D, L + 1]
    reps, final = rep[:, :, :-1], rep[:, :, -1]

    def score(ids):
        return F.embedding(ids, b, padding_idx=0).squeeze(-1) + (reps * vectors(ids).permute(0, 2, 1)).sum(1)

    sp = score(seqs)
    sc = torch.stack([score(cand[r]) for r in range(nn)])
    first = torch.from_numpy(np.argmax(sc.detach().numpy(), axis=0))  # the first maximum, as the restatement takes it
    sn = torch.gather(sc, 0, first.unsqueeze(0))[0]
    if case.loss == 'bpr':
        l = 1.0 - torch.sigmoid(sp - sn)
    elif case.loss == 'pointwise':
        l = (1.0 - torch.sigmoid(sp)) + torch.sigmoid(sn)
    else:
        l = torch.clamp(sn - sp + 1.0, 0.0)
    mask = (seqs != 0).double()
    loss = (l * mask).sum() / mask.sum()
    loss.backward()
    return float(loss.detach()), reps.permute(0, 2, 1).detach().numpy(), final.detach().numpy(), E.grad.numpy(), b.grad.numpy().ravel()


def close(got, want, scale, what):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    assert (d <= RTOL * scale).all(), (what, float((d / np.where(scale > 0, scale, 1.0)).max()))


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_against_torch_autograd_in_float64(name):
    case = CASES[name]()
    x = case.exact
    loss, rep, final, g_rows, g_bias = torch_minibatch(case)
    assert abs(loss - float(x.loss)) <= RTOL * x.loss_mag
    scale = np.abs(rep).max()
    close(x.rep, rep, scale, 'representations')
    close(x.rep_final, final, scale, 'final representation')
    # each row against the float64 sum of |terms| it is made of (mag); exactly zero where that is zero
    close(x.grad_rows, g_rows, x.mag_rows[:, None], 'item rows')
    close(x.grad_bias, g_bias, x.mag_bias, 'item biases')
    # and the yardstick is a float32 evaluation of the same thing: it is close, and it is not the same numbers
    assert 0 < max(case.yard_rows, case.yard_bias) <= sx.YARD_MAX


def test_restatement_without_a_real_entry_against_torch():
    case = sx.no_real_entry_case()
    x = case.exact
    loss, _, _, g_rows, g_bias = torch_minibatch(case)
    assert np.isnan(loss) and np.isnan(x.loss)
    assert np.array_equal(np.isnan(g_rows), np.isnan(x.grad_rows)) and np.array_equal(np.isnan(g_bias), np.isnan(x.grad_bias))
    assert np.isnan(x.grad_rows[case.negs]).all() and (g_rows[~np.isnan(g_rows)] == 0).all()


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_against_the_oracle(name):
    """PoolNetOracle (float32 C) at its usual bound -- 1e-5 of each table's inf-norm, 1e-4 where rows sum thousands of terms: a
    sanity check of the comparison only."""
    from oracle.oracle import PoolNetOracle
    case = CASES[name]()
    x = case.exact
    want_loss, want_g = PoolNetOracle(case.E, case.bias, opt='adagrad', item_bloom=case.bloom).step(
        case.seqs, case.negs, loss=case.loss, n_neg=case.n_neg, want_grads=True)
    tol = 1e-4 if name.startswith('shared') else 1e-5
    assert abs(want_loss - float(x.loss)) <= 1e-5 * abs(float(x.loss))
    assert np.abs(want_g[0] - x.grad_rows).max() <= tol * np.abs(x.grad_rows).max()
    assert np.abs(want_g[1].ravel() - x.grad_bias).max() <= tol * np.abs(x.grad_bias).max()


LIVE_SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
from oracle.reference_import import import_reference
import_reference()
import numpy as np
import torch
from spotlight.sequence.representations import PoolNet
from spotlight.layers import BloomEmbedding
from spotlight import losses
rec = np.load(%(inp)r)
E, bias, seqs, negs = rec['E'], rec['bias'], rec['seqs'], rec['negs']
loss_name, n_neg, n_hash = str(rec['loss']), int(rec['n_neg']), int(rec['n_hash'])
I, (rows, D) = bias.size, E.shape
layer = None
if n_hash:
    layer = BloomEmbedding(I, D, compression_ratio=(rows + 0.5) / I, num_hash_functions=n_hash, padding_idx=0)
    assert layer.compressed_num_embeddings == rows
net = PoolNet(I, D, item_embedding_layer=layer).double()
table = net.item_embeddings.embeddings if n_hash else net.item_embeddings
with torch.no_grad():
    table.weight.copy_(torch.from_numpy(E.astype(np.float64)))
    net.item_biases.weight.copy_(torch.from_numpy(bias.astype(np.float64).reshape(-1, 1)))
s = torch.from_numpy(seqs)
B, L = seqs.shape
rep, final = net.user_representation(s)
pos = net(rep, s)
if loss_name == 'adaptive_hinge':
    neg = net(rep.repeat(n_neg, 1, 1), torch.from_numpy(negs.reshape(n_neg * B, L))).view(n_neg, B, L)
else:
    neg = net(rep, torch.from_numpy(negs.reshape(B, L)))
fn = dict(pointwise=losses.pointwise_loss, bpr=losses.bpr_loss, hinge=losses.hinge_loss, adaptive_hinge=losses.adaptive_hinge_loss)[loss_name]
loss = fn(pos, neg, mask=(s != 0))
loss.backward()
np.savez(%(out)r, loss=loss.item(), rep=rep.detach().numpy(), final=final.detach().numpy(), g_rows=table.weight.grad.numpy(),
         g_bias=net.item_biases.weight.grad.numpy().ravel())
'''

LIVE_CASES = [n for n in sorted(CASES) if n != 'tie']  # (what torch.max does with equal scores is not the reference's statement)


@pytest.mark.skipif(not LIVE, reason='needs the live reference (/root/reference: build container only)')
@pytest.mark.parametrize('name', LIVE_CASES)
def test_restatement_against_the_live_reference_in_float64(name, tmp_path):
    """The reference's own PoolNet, BloomEmbedding and loss functions, in float64, in an interpreter of their own."""
    case = CASES[name]()
    x = case.exact
    inp, out = str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')
    np.savez(inp, E=case.E, bias=case.bias, seqs=case.seqs, negs=case.negs, loss=case.loss, n_neg=case.n_neg,
             n_hash=case.bloom['n_hash'] if case.bloom else 0)
    r = subprocess.run([sys.executable, '-c', LIVE_SCRIPT % dict(root=ROOT, inp=inp, out=out)], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(out)
    assert abs(float(got['loss']) - float(x.loss)) <= RTOL * x.loss_mag
    scale = np.abs(x.rep).max()
    close(x.rep, got['rep'].transpose(0, 2, 1), scale, 'representations')
    close(x.rep_final, got['final'], scale, 'final representation')
    close(x.grad_rows, got['g_rows'], x.mag_rows[:, None], 'item rows')
    close(x.grad_bias, got['g_bias'], x.mag_bias, 'item biases')
