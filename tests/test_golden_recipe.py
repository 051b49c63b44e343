"""Guards of the parity recipe: the fixture generators under oracle/ must run THE REFERENCE, never
this repository's `spotlight/` alias package onto the product, and -- wherever the live reference exists -- regenerating
the fixtures must reproduce tests/golden bit for bit.  CPU only; each generator runs in its own interpreter."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATORS = ['make_golden', 'make_golden_seq', 'make_golden_bloom', 'make_golden_explicit', 'make_golden_encoders',
              'make_golden_host', 'make_golden_floors']
LIVE = os.path.isfile('/root/reference/spotlight/__init__.py')
STAGED = os.path.isfile(os.path.join(ROOT, 'oracle', '_ref', 'spotlight', '__init__.py'))

# Where the reference exists neither live nor staged, the import routing is checked against a stand-in written under the
# test's tmp_path: a package with the reference's module names, whose leaf modules hand out a placeholder class for any
# name and whose modules all import a sibling by its absolute `spotlight.` name, as the reference's own modules do.
STAND_IN_PACKAGES = ['', 'factorization', 'sequence', 'datasets']
STAND_IN_MODULES = ['interactions', 'layers', 'losses', 'torch_utils', 'cross_validation', 'evaluation', 'factorization/implicit',
                    'factorization/explicit', 'factorization/representations', 'sequence/implicit', 'sequence/representations',
                    'datasets/synthetic']


def _stand_in_reference(root):
    pkg = root / 'spotlight'
    for sub in STAND_IN_PACKAGES:
        (pkg / sub).mkdir(parents=True, exist_ok=True)
        (pkg / sub / '__init__.py').write_text('import spotlight.losses\n')
    for mod in STAND_IN_MODULES:
        (pkg / (mod + '.py')).write_text('import spotlight.losses\n\n\n'
                                         'def __getattr__(name):\n'
                                         '    if name.startswith("__"):\n'
                                         '        raise AttributeError(name)\n'
                                         '    return type(name, (), {})\n')
    return str(root)


def _run(code, cwd=ROOT, env=None):
    e = dict(os.environ)
    e.pop('SLK_GOLDEN_OUT', None)
    e.update(env or {})
    return subprocess.run([sys.executable, '-c', code], cwd=cwd, env=e, capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('gen', GENERATORS)
def test_generator_imports_the_reference_not_the_product(gen, tmp_path):
    # importing the generator module (not running it) performs its imports; cwd = repository root, i.e. the alias
    # package `spotlight/` is first on sys.path -- exactly the situation in which the old recipe loaded the product
    code = ('import sys, importlib; sys.path.insert(0, %r)\n'
            'm = importlib.import_module("oracle.%s")\n'
            'import spotlight\n'
            'from oracle.reference_import import assert_is_reference\n'
            'assert_is_reference(spotlight)\n'
            'mods = [n for n in sys.modules if n == "spotlight_amd" or n.startswith("spotlight_amd.")]\n'
            'assert not mods, mods\n'
            'for n, mod in list(sys.modules.items()):\n'
            '    if n.startswith("spotlight.") and mod is not None: assert_is_reference(mod)\n'
            'print("REFERENCE", spotlight.__file__)\n') % (ROOT, gen)
    r = _run(code, env=None if (LIVE or STAGED) else {'SPOTLIGHT_REFERENCE': _stand_in_reference(tmp_path)})
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'REFERENCE' in r.stdout and 'spotlight_amd' not in r.stdout.split('REFERENCE')[-1]


def test_guard_rejects_the_alias_package():
    # the guard itself must fire on the product's alias (without needing a HIP device: the alias module is faked)
    code = ('import sys, types; sys.path.insert(0, %r)\n'
            'fake = types.ModuleType("spotlight"); fake.__file__ = %r\n'
            'sys.modules["spotlight"] = fake\n'
            'from oracle.reference_import import import_reference\n'
            'try:\n'
            '    import_reference()\n'
            'except (AssertionError, RuntimeError) as e:\n'
            '    print("REJECTED")\n'
            'else:\n'
            '    raise SystemExit("the alias package was accepted as the reference")\n') % (
                ROOT, os.path.join(ROOT, 'spotlight', '__init__.py'))
    r = _run(code)
    assert r.returncode == 0 and 'REJECTED' in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(not LIVE, reason='regeneration needs the live reference (/root/reference: build container only)')
@pytest.mark.parametrize('gen,args', [('make_golden', []), ('make_golden_seq', []), ('make_golden_seq', ['bloom']),
                                      ('make_golden_bloom', []), ('make_golden_explicit', []),
                                      ('make_golden_encoders', []), ('make_golden_host', [])])
def test_regenerated_fixtures_are_bit_identical(gen, args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'oracle', gen + '.py'), '--check'] + args, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'bit-identical to tests/golden' in r.stdout
