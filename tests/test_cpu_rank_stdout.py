"""The ranks of a job share the launcher's stdout, and the gloo library announces each rank's connections there in several writes
per line: while the process group is built, file descriptor 1 points at stderr (parallel._stdout_to_stderr), so no fragment of a
banner lands between the lines of a command whose stdout is its result."""
import os
import subprocess
import sys

from conftest import ROOT

CHILD = r'''
import os, sys
from topaz_amd.parallel import _stdout_to_stderr
print('before')                                  # (buffered by Python: must come out BEFORE the block's raw writes)
with _stdout_to_stderr():
    os.write(1, b'[Gloo] Rank 0 is ')            # what a C++ library does: raw writes to descriptor 1
    os.write(1, b'connected\n')
os.write(1, b'after raw\n')
print('after')
'''


def _run(code, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    return subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120, **kw)


def test_descriptor_1_points_at_stderr_inside_the_block_only():
    r = _run(CHILD)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == 'before\nafter raw\nafter\n'
    assert '[Gloo] Rank 0 is connected\n' in r.stderr


def test_world_of_one_gloo_group_leaves_stdout_to_the_command():
    """a real process group (gloo, one rank, forced): whatever the library prints while connecting, stdout holds the command's own
    lines only and still works afterwards"""
    code = ('import os\n'
            'os.environ.update(TOPAZ_AMD_FORCE_DIST="1", TOPAZ_AMD_DIST_BACKEND="gloo", MASTER_PORT="29577")\n'
            'from topaz_amd import parallel\n'
            'print("# result line 1")\n'
            'print(parallel.init_from_env())\n'
            'print("# result line 2")\n')
    r = _run(code)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == '# result line 1\n(0, 0, 1)\n# result line 2\n'
