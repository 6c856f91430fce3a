"""bench.py's command line (no GPU): a plain run has every side figure and check switched off, `--full` has
them on and the --no-* options still trim it.  The parsing runs in a child process, so that importing bench.py
leaves this process's environment alone."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = ('no_cpu', 'no_example', 'no_extras', 'no_configs', 'no_multi')


def parsed(*argv):
    code = ('import json, sys, bench; a = bench.parse_args(sys.argv[1:]); '
            'print(json.dumps({k: getattr(a, k) for k in %r + ("full", "steps", "warmup")}))' % (SIDE,))
    out = subprocess.check_output([sys.executable, '-c', code] + list(argv), cwd=ROOT, text=True)
    return json.loads(out.strip().splitlines()[-1])


def test_plain_run_measures_the_headline_only():
    a = parsed('--gpus', '1', '--steps', '7', '--warmup', '2')
    assert a['full'] is False
    assert all(a[k] is True for k in SIDE), a
    assert (a['steps'], a['warmup']) == (7, 2)


def test_full_run_keeps_every_side_figure():
    a = parsed('--gpus', '1', '--steps', '7', '--warmup', '2', '--full')
    assert a['full'] is True
    assert not any(a[k] for k in SIDE), a
    a = parsed('--full', '--no-cpu', '--no-example')
    assert (a['no_cpu'], a['no_example'], a['no_extras'], a['no_configs'], a['no_multi']) == \
        (True, True, False, False, False)
