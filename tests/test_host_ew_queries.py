"""CPU-only guard of the host layer of norm.hip, elementwise.hip, binarize.hip and metrics.hip: the workspace-size and
partial-count queries must answer what tests/golden/ew_host_queries.json recorded (every InstanceNorm of the three bench
configurations, both PatchGAN scales, the 2048x1024 sizes and the norm shapes tests/test_hip_ops.py parametrises, bf16 and
fp32), and every recorded bad call -- bad dtype, null pointer, non-positive extent, count that is not a vector multiple,
workspace one byte short, has_residual without a residual, zero slots -- must still be refused with the same return code and
the same jpdse_last_error() text.  The fixture is written by scripts/make_ew_host_queries.py.  Nothing is launched: the replay
runs that script in a child process that sees no GPU, so a call a broken build failed to refuse could not reach a device."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, 'scripts', 'make_ew_host_queries.py')
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def launching_entry_points():
  """Entry points of include/jpdse.h that enqueue work on a stream, the conv family (conv_gemm.hip) excepted."""
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  names = {m.group(1) for m in re.finditer(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(([^)]*)\)\s*;', header) if 'void* stream' in m.group(2)}
  return {n for n in names if not n.startswith(('jpdse_conv_', 'jpdse_convT_'))}


def test_ew_host_queries_match_the_recorded_answers(tmp_path):
  import make_ew_host_queries as gen
  fix = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'ew_host_queries.json')))
  assert fix['slope'] == gen.SLOPE and fix['eps'] == gen.EPS
  # the fixture covers exactly the list the generator would write today (a case added there needs a regenerated fixture)
  assert [c[:2] for c in fix['answers']] == gen.answer_keys()
  assert [c[:3] for c in fix['refusals']] == gen.refusals()
  assert len(fix['answers']) >= 300 and sum(1 for c in fix['answers'] if c[0] == 'jpdse_inorm_workspace_size') >= 200
  # at least one refusal for every launching entry point of the four files, each a bad argument or a short workspace
  entry_points = launching_entry_points()
  assert len(entry_points) >= 34
  refused = {c[0] for c in fix['refusals']}
  assert refused == entry_points, 'no recorded refusal: %s; not a launching entry point: %s' % (
      sorted(entry_points - refused), sorted(refused - entry_points))
  assert all(c[3] in (-1, -2) and c[4] for c in fix['refusals'])
  # replay with the in-tree library
  out = str(tmp_path / 'ew_host_queries.json')
  env = {k: v for k, v in os.environ.items() if k != 'JPDSE_HIP_LIB'}
  python = [sys.executable] + (['-s'] if sys.flags.no_user_site else [])
  run = subprocess.run(python + [SCRIPT, out], env=env, capture_output=True, text=True)
  assert run.returncode == 0, run.stdout + run.stderr
  got = json.load(open(out))
  wrong = ['%s%s: %s, recorded %s' % (w[0], w[1], g[2], w[2]) for g, w in zip(got['answers'], fix['answers']) if g != w]
  wrong += ['%s (%s): %s, recorded %s' % (w[0], w[1], g[3:], w[3:]) for g, w in zip(got['refusals'], fix['refusals']) if g != w]
  assert not wrong, '%d answers differ:\n%s' % (len(wrong), '\n'.join(wrong[:20]))
  assert got == fix
