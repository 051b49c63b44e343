"""bench.py's launch logic on a box without GPUs: `--backend emu` runs the same host code (argument handling,
self-spawn of N ranks through torch.distributed.run, the sharded trainer loop, max-over-ranks timing, the JSON line)
over gloo and the emulator build of the kernels.  The numbers are meaningless; the structure is what is checked."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
SMALL = ['--backend', 'emu', '--users', '3000', '--items', '700', '--dim', '16', '--batch', '256', '--steps', '2',
         '--warmup', '1', '--no-cpu-baseline']


def run_bench(extra, env_extra=None, timeout=900):
    from emu_backend import emu_lib
    emu_lib()  # build once, before several ranks race for it
    env = dict(os.environ, OMP_NUM_THREADS='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, BENCH] + SMALL + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                       timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


EXTRAS = ('roofline', 'ms_per_step_with_kernel_timers', 'sharded_world1_consistency', 'fit_end_to_end', 'cpu_baseline', 'configs')


def test_plain_run_prints_the_headline_line_and_nothing_that_takes_a_run_of_its_own():
    """Without --full: one JSON line with the contract fields, none of the objects that --full adds -- and the --no-* options,
    which take pieces out of a --full run, change nothing about it."""
    for extra in ([], ['--no-probes', '--no-sharded-check', '--no-fit', '--no-configs', '--no-denominators']):
        rc, out, err = run_bench(['--gpus', '1'] + extra)
        assert rc == 0, err[-3000:]
        lines = [l for l in out.splitlines() if l.strip()]
        assert len(lines) == 1, out
        rec = json.loads(lines[0])
        for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                    'vs_baseline', 'dtype', 'data', 'config', 'first_call', 'final_minibatch_loss'):
            assert key in rec, key
        assert rec['full'] is False and not [k for k in EXTRAS if k in rec], sorted(rec)
        assert rec['n_gpus'] == 1 and rec['steps'] == 2 and rec['warmup'] == 1 and rec['higher_is_better'] is True
        assert rec['ms_per_step'] > 0 and abs(rec['value'] * rec['ms_per_step'] * 1e-3 - 256) < 1e-6 * 256  # = batch / step time
        assert rec['ranks']['world_size_observed'] == 1 and rec['final_minibatch_loss'] > 0


def test_plain_n_gpu_run_has_no_denominators():
    rc, out, err = run_bench(['--gpus', '2'])
    assert rc == 0, err[-3000:]
    rec = json.loads([l for l in out.splitlines() if l.strip().startswith('{')][-1])
    assert rec['n_gpus'] == 2 and rec['ranks']['world_size_observed'] == 2 and rec['full'] is False
    assert not [k for k in EXTRAS if k in rec], sorted(rec)
    assert all(d['exchange_rows_timed_call'] > 0 for d in rec['ranks']['devices']) and rec['final_minibatch_loss'] > 0


def test_single_rank_line_has_the_contract_fields():
    rc, out, err = run_bench(['--gpus', '1', '--full'])
    assert rc == 0, err[-3000:]
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out  # exactly ONE JSON line on stdout
    rec = json.loads(lines[0])
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config', 'roofline'):
        assert key in rec, key
    assert rec['n_gpus'] == 1 and rec['steps'] == 2 and rec['warmup'] == 1 and rec['vs_baseline'] is None
    roof = rec['roofline']
    for key in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'measured', 'ceiling'):
        assert key in roof, key
    assert roof['measured']['copy_GBs'] > 0 and roof['ceiling']['ms_per_step'] > 0
    assert rec['full'] is True and rec['ms_per_step_with_kernel_timers'] > 0
    chk = rec['sharded_world1_consistency']
    assert chk.get('consistent') is True, chk
    assert rec['ranks']['world_size_observed'] == 1


@pytest.mark.parametrize('n', [2, 4])
def test_gpus_n_spawns_n_ranks_itself(n):
    """`python bench.py --gpus N` with no torchrun environment launches the N ranks itself (--full: the line's xGMI accounting
    and rank 0's one-GPU denominators)."""
    rc, out, err = run_bench(['--gpus', str(n), '--full'])
    assert rc == 0, err[-3000:]
    lines = [l for l in out.splitlines() if l.strip().startswith('{')]
    assert len(lines) == 1, out
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == n and rec['ranks']['world_size_observed'] == n
    assert sorted(d['rank'] for d in rec['ranks']['devices']) == list(range(n))
    assert rec['ranks']['launched_by'].startswith('bench.py')
    assert rec['config']['global_batch'] == 256 * n and rec['scaling'] == 'weak'
    xg = rec['roofline']['xgmi']
    assert xg['rows_per_step_per_gpu'] > 0
    # the curve's stated bound and denominators: the wire bound of this world size, and rank 0's own
    # world-1 runs of the same per-GPU shape through the fused and the row-sharded path
    assert xg['bound_%d_gpus' % n]['interactions_per_s_at_link_peak'] > 0
    den = xg['denominators_1_gpu']
    assert den['fused']['interactions_per_s'] > 0 and den['sharded_world1']['interactions_per_s'] > 0
    assert abs(den['fused']['scaling_factor_of_this_run'] * den['fused']['interactions_per_s'] - rec['value']) < 1e-6 * rec['value']


@pytest.mark.parametrize('n', [2, 3])
def test_default_n_gpu_configuration_c5_at_reduced_rows(n):
    """what `bench.py --gpus N` runs by DEFAULT at N > 1 -- the C5 row-sharded configuration -- end to end
    at reduced rows: the line names the workload, the process group saw N ranks, every rank reports the lookups it sent to other
    ranks (about (N - 1) / N of its 2 B K), and rank 0's own world-1 runs of the same per-GPU shape -- fused path and
    row-sharded path -- agree on every minibatch's loss."""
    rc, out, err = run_bench(['--gpus', str(n), '--workload', 'c5', '--full'])
    assert rc == 0, err[-3000:]
    rec = json.loads([l for l in out.splitlines() if l.strip().startswith('{')][-1])
    assert rec['config']['workload'].startswith('C5') and 'row-sharded x%d' % n in rec['config']['parallelism']
    assert rec['n_gpus'] == n and rec['ranks']['world_size_observed'] == n
    devs = sorted(rec['ranks']['devices'], key=lambda d: d['rank'])
    assert [d['rank'] for d in devs] == list(range(n))
    lookups = 2 * 256 * rec['steps']
    for d in devs:
        share = d['exchange_rows_timed_call'] / lookups
        assert abs(share - (n - 1) / n) < 0.12, (d, share)
    assert abs(sum(d['exchange_rows_timed_call'] for d in devs) / n / rec['steps'] - rec['roofline']['xgmi']['rows_per_step_per_gpu']) <= \
        max(d['exchange_rows_timed_call'] for d in devs) / rec['steps']
    # MEASURED wire bytes: what every rank's trainer handed to the collectives for other ranks.  A rank sends
    # the ids (4 B) and gradient rows ((D + 1) floats) of ITS remote lookups and the rows ((D + 1) floats) of the lookups OTHER
    # ranks make of it, so over all ranks the payload is EXACTLY remote lookups x (4 + 2 (D + 1) 4) bytes -- the per-lookup figure
    # behind DESIGN.md section 7's 0.92 KB per interaction (2 lookups x 7/8 remote x 524 B at D = 64); per rank it differs from
    # the line's model (rank 0's own remote lookups x the same figure) only by the imbalance of the uniform draw.  What left with
    # the slot padding (whole blocks of 64 slots per peer and unit) is at least the payload.
    D = 16
    per_lookup = 4 + 2 * (D + 1) * 4
    assert sum(d['exchange_payload_bytes_timed_call'] for d in devs) == sum(d['exchange_rows_timed_call'] for d in devs) * per_lookup
    for d in devs:
        assert abs(d['exchange_payload_bytes_timed_call'] - d['exchange_rows_timed_call'] * per_lookup) <= 0.1 * d['exchange_payload_bytes_timed_call'], d
        assert d['exchange_payload_bytes_timed_call'] <= d['exchange_bytes_timed_call']
    xg = rec['roofline']['xgmi']
    assert xg['bytes_per_step_per_gpu_each_way'] == xg['rows_per_step_per_gpu'] * per_lookup  # the model: rank 0's remote lookups x the figure
    assert abs(xg['payload_bytes_per_step_per_gpu_each_way_measured'] - xg['bytes_per_step_per_gpu_each_way']) <= 0.1 * xg['bytes_per_step_per_gpu_each_way']
    den = rec['roofline']['xgmi']['denominators_1_gpu']
    a, b = den['fused']['minibatch_losses'], den['sharded_world1']['minibatch_losses']
    assert len(a) == len(b) == rec['steps'] + rec['warmup'] and all(x > 0 for x in a)
    assert max(abs(x - y) for x, y in zip(a, b)) <= 1e-5 * max(a), (a, b)


def test_row_sharded_bench_loop_on_the_bias_shadow():
    """`bench.py --gpus 2` at item-table sizes where the run trains with {item bias, Adagrad accumulator} interleaved (forced at
    reduced rows): the same per-minibatch loss as the plain layout -- same seeds, same draws --, and the line says which layout ran."""
    final = []
    for extra in (['--bias-shadow-min-items', '1'], ['--no-bias-shadow']):
        rc, out, err = run_bench(['--gpus', '2', '--workload', 'c5', '--full'] + extra)
        assert rc == 0, err[-3000:]
        rec = json.loads([l for l in out.splitlines() if l.strip().startswith('{')][-1])
        assert rec['config']['item_bias_layout'].startswith('two arrays') == (extra[0] == '--no-bias-shadow')
        final.append(rec['final_minibatch_loss'])
        # rank 0's own one-GPU runs of the per-GPU shape (the row-sharded one on the same bias layout as the N-GPU run) agree
        den = rec['roofline']['xgmi']['denominators_1_gpu']
        a, b = den['fused']['minibatch_losses'], den['sharded_world1']['minibatch_losses']
        assert max(abs(x - y) for x, y in zip(a, b)) <= 1e-5 * max(a), (a, b)
    assert final[0] == final[1] and final[0] > 0


def test_dump_outputs_of_the_last_timed_step(tmp_path):
    """`--dump-outputs DIR`: float32 / float64 .npy files of at most 64 MB holding the last timed call's K minibatch losses and
    sampled rows of the tables and optimizer state; the same arguments give the same inputs, so two runs write the same arrays."""
    import numpy as np
    dumps = []
    for run in ('a', 'b'):
        d = tmp_path / run
        rc, out, err = run_bench(['--gpus', '1', '--steps', '3', '--dump-outputs', str(d)])
        assert rc == 0, err[-3000:]
        rec = json.loads([l for l in out.splitlines() if l.strip().startswith('{')][-1])
        assert rec['steps'] == 3 and rec['ms_per_step'] > 0
        arrs = {f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(d)) if f.endswith('.npy')}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        loss = arrs['minibatch_losses']
        assert loss.shape == (3,) and loss[-1] == np.float32(rec['final_minibatch_loss']) and (loss > 0).all()
        assert arrs['user_embeddings'].shape == arrs['item_embeddings'].shape == (256, 16)
        assert arrs['item_biases_opt_state1'].shape == (256,) and (arrs['item_biases_opt_state1'] > 0).all()  # every sampled row stepped
        dumps.append(arrs)
    assert sorted(dumps[0]) == sorted(dumps[1])
    for name in dumps[0]:
        np.testing.assert_array_equal(dumps[0][name], dumps[1][name], err_msg=name)


def test_full_run_trains_what_a_plain_run_trains(tmp_path):
    """--full adds measurements around the training calls, never a training step: same losses, same dumped arrays, bit for bit."""
    import numpy as np
    dumps, final = [], []
    for name, extra in (('plain', []), ('full', ['--full'])):
        d = tmp_path / name
        rc, out, err = run_bench(['--gpus', '1', '--steps', '3', '--dump-outputs', str(d)] + extra)
        assert rc == 0, err[-3000:]
        rec = json.loads([l for l in out.splitlines() if l.strip().startswith('{')][-1])
        assert rec['full'] is (name == 'full') and ('roofline' in rec) == (name == 'full')
        final.append(rec['final_minibatch_loss'])
        dumps.append({f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(d)) if f.endswith('.npy')})
    assert final[0] == final[1] and sorted(dumps[0]) == sorted(dumps[1]) and 'minibatch_losses' in dumps[0]
    for name in dumps[0]:
        np.testing.assert_array_equal(dumps[0][name], dumps[1][name], err_msg=name)


def test_dump_outputs_refuses_other_workloads():
    rc, out, err = run_bench(['--gpus', '1', '--workload', 'c4', '--dump-outputs', 'unused'])
    assert rc != 0 and '--dump-outputs' in err and not out.strip()


def test_world_size_mismatch_fails_loudly():
    rc, out, err = run_bench(['--gpus', '2'], env_extra={'WORLD_SIZE': '1', 'RANK': '0', 'LOCAL_RANK': '0'})
    assert rc != 0 and 'WORLD_SIZE' in err and not out.strip()


def test_hip_backend_refuses_more_ranks_than_gpus():
    """On this GPU-less box the product backend must refuse `--gpus 2` instead of running fewer ranks."""
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip('box has >= 2 GPUs')
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, BENCH, '--gpus', '2', '--steps', '1', '--warmup', '0'], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=env, timeout=300)
    assert p.returncode != 0 and b'refusing' in p.stderr and not p.stdout.strip()


def test_adaptive_hinge_on_the_row_sharded_bench_path():
    """`--loss adaptive_hinge` at N > 1 (the reference's default of 5 draws per interaction travels with the call): the line
    comes out and the ranks' loss shares add up to a finite, positive minibatch loss."""
    rc, out, err = run_bench(['--gpus', '2', '--loss', 'adaptive_hinge', '--no-denominators'])
    assert rc == 0, err[-3000:]
    rec = json.loads([l for l in out.splitlines() if l.strip().startswith('{')][-1])
    assert rec['n_gpus'] == 2 and rec['ranks']['world_size_observed'] == 2
    assert 'adaptive_hinge' in rec['config']['workload'] and rec['final_minibatch_loss'] > 0
