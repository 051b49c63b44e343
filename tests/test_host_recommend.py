"""recommend() of the models through the emulator build of the kernels (no GPU), and of the row-sharded model over gloo at world
2 and 3 (tests/shard_topk_worker.py).  The same checks run on the gfx950 library in tests/test_gpu_recommend.py."""
import os

import pytest
import torch

import recommend_checks as rc
from emu_backend import emu_lib
from spotlight_amd import _native
from spotlight_amd.factorization import implicit as host
from test_sharded import run_world

HERE = os.path.dirname(os.path.abspath(__file__))
TOPK_WORKER = os.path.join(HERE, 'shard_topk_worker.py')


@pytest.fixture()
def emu_device(monkeypatch):
    eng = _native.Engine(0, lib=emu_lib())
    monkeypatch.setattr(host, '_engine_for', lambda device: eng)
    monkeypatch.setattr(host, '_stream_for', lambda device: 0)
    monkeypatch.setattr(host, '_model_device', lambda: torch.device('cpu'))
    yield eng
    eng.close()


def test_bilinear_recommend(emu_device):
    rc.check_bilinear_recommend()


def test_poolnet_recommend(emu_device):
    rc.check_poolnet_recommend()


def test_native_refuses_an_older_library():
    class Old(object):
        def __getattr__(self, name):
            class F(object):
                restype = argtypes = None

                def __call__(self, *a):
                    return 13
            return F()
    with pytest.raises(ImportError, match='ABI 13 != expected 14'):
        _native.bind(Old())


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_recommend_matches_single_device_model(world):
    run_world(world, [], worker=TOPK_WORKER, token='SHARD_TOPK_OK', timeout=240)
