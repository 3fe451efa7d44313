'''CPU-side checks of the drop-in boundary: the shared library loads and exports
every symbol include/nutils_hip.h declares (no compute calls without a GPU), and
the ctypes signature table covers exactly that set.'''
import ctypes
import os
import re
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared():
    src = open(os.path.join(ROOT, 'include', 'nutils_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(nh_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    from nutils_amd import _lib
    assert os.path.exists(_lib.LIBPATH), 'run __graft_entry__.build() first'
    lib = ctypes.CDLL(_lib.LIBPATH)
    names = declared()
    assert len(names) >= 20
    for name in names:
        assert hasattr(lib, name), name
    assert lib.nh_abi_version() == 1


def test_ctypes_table_matches_header():
    from nutils_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared()


def test_error_reporting_without_gpu():
    from nutils_amd import _lib
    lib = _lib.load()
    # an invalid argument is reported through the status code + nh_last_error, never a crash
    rc = lib.nh_poly_tabulate(None, 1, 7, None, 1, 3, None, None)
    assert rc == -1
    assert b'not a valid coefficient count' in lib.nh_last_error()
    with pytest.raises(_lib.NutilsHipError):
        _lib.check(rc)


def _register():
    '''The tables of INTEGRATION.md section 5: {'5.1': names, '5.2': names, '5.3': names} (first column of every table row).'''
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    text = text[text.index('\n## 5. '):text.index('\n## 6. ')]
    tables = {}
    for part in re.split(r'\n### ', text)[1:]:
        rows = [line.split('|')[1] for line in part.split('\n') if line.startswith('| `')]
        tables[part[:3]] = {name for row in rows for name in re.findall(r'`((?:NH|NUTILS_AMD|NUTILS_HIP)_[A-Z0-9_]+)', row)}
    return tables


def test_environment_switches_match_their_register():
    '''INTEGRATION.md section 5 is the register of environment switches.  The default library holds exactly the names of 5.2 (as NUL-delimited strings:
    a tuning variable left in a shell cannot reach a shipped kernel), the names the sources pass to getenv beyond those are the ablation-only ones
    of 5.3, and the Python package reads the names of 5.1.'''
    tables = _register()
    assert sorted(tables) == ['5.1', '5.2', '5.3']
    path = os.path.join(ROOT, 'nutils_amd', 'libnutils_hip.so')
    assert os.path.exists(path), 'run __graft_entry__.build() first'
    in_library = {m.decode() for m in re.findall(rb'(?<=\0)(?:NH|NUTILS_AMD)_[A-Z0-9_]+(?=\0)', open(path, 'rb').read())}
    assert in_library == tables['5.2']
    csrc = os.path.join(ROOT, 'nutils_amd', 'csrc')
    in_sources = set()
    for name in os.listdir(csrc):
        if name.endswith(('.hip', '.inc', '.h')):
            in_sources |= set(re.findall(r'getenv\("([A-Z0-9_]+)"\)', open(os.path.join(csrc, name)).read()))
    assert in_library <= in_sources
    assert in_sources - in_library == tables['5.3']
    in_python = set()
    pkg = os.path.join(ROOT, 'nutils_amd')
    for name in os.listdir(pkg):
        if name.endswith('.py'):
            src = open(os.path.join(pkg, name)).read()
            assert len(re.findall(r'\benviron\b', src)) == len(re.findall(r"os\.environ\.get\('", src)), \
                f"{name}: read switches as os.environ.get('NAME') (and spell the word otherwise in comments), so that this test sees every read"
            in_python |= set(re.findall(r"os\.environ\.get\('([A-Z0-9_]+)'[,)]", src))
            for prefix, names in re.findall(r"os\.environ\.get\('([A-Z0-9_]+)' \+ name\)\) for name in \(([^)]*)\)", src):
                in_python |= {prefix + n for n in re.findall(r"'([A-Z0-9_]+)'", names)}
    assert in_python == tables['5.1']
