#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code objects of two builds of jpd-se_amd/csrc (a change of the host layer must leave
them alone; it is what stands in for "kernel speed unchanged").

  python scripts/diff_code_objects.py CSRC_DIR_A CSRC_DIR_B

CSRC_DIR_x: a csrc directory after `make` (it holds conv_gemm.o, conv_gemm.dev.o, norm.o, norm.dev.o, elementwise.o,
binarize.o, metrics.o).  Per object file the gfx950 code object is taken out of the .hip_fatbin section (llvm-objcopy +
clang-offload-bundler), then compared PER SYMBOL -- host code that instantiates kernels in another order may reorder them
inside the object:
  * the set of kernels (the .kd symbols),
  * the resources of each (vgpr / sgpr / agpr count, LDS and scratch size, kernarg size: the metadata note),
  * the instruction stream of each function (llvm-objdump -d, addresses and encodings stripped).
Exit status 0 when nothing differs, 1 otherwise."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM_BIN', '/opt/rocm/llvm/bin')
OBJECTS = ['conv_gemm.o', 'conv_gemm.dev.o', 'norm.o', 'norm.dev.o', 'elementwise.o', 'binarize.o', 'metrics.o']
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
RESOURCES = ('.vgpr_count', '.sgpr_count', '.agpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size',
             '.kernarg_segment_size')


def tool(name, *args):
  return subprocess.run((os.path.join(LLVM, name),) + args, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
  fat, co = os.path.join(tmp, 'x.fat'), os.path.join(tmp, 'x.co')
  tool('llvm-objcopy', '-O', 'binary', '--only-section=.hip_fatbin', obj, fat)
  tool('clang-offload-bundler', '--unbundle', '--type=o', '--input=' + fat, '--targets=' + TARGET, '--output=' + co)
  return co


def read_code_object(co):
  """(kernel names, {kernel: resources}, {function symbol: [instructions]})"""
  kernels = set()
  for line in tool('llvm-readelf', '-s', '--wide', co).splitlines():
    f = line.split()
    if len(f) >= 8 and f[3] == 'OBJECT' and f[7].endswith('.kd'):
      kernels.add(f[7][:-3])
  resources, cur = {}, None
  for line in tool('llvm-readelf', '--notes', co).splitlines():
    m = re.match(r'^  - (\.\w+):\s*(.*)$', line)          # first key of an entry of amdhsa.kernels
    if m:
      cur = {}
    else:
      m = re.match(r'^    (\.\w+):\s*(.*)$', line)        # its other top-level keys
    if m and cur is not None:
      cur[m.group(1)] = m.group(2).strip()
      if m.group(1) == '.symbol':
        resources[cur['.symbol'].strip('\'"')[:-3]] = cur
  resources = {k: tuple(v.get(r) for r in RESOURCES) for k, v in resources.items()}
  code, cur = {}, None
  for line in tool('llvm-objdump', '-d', '--no-show-raw-insn', '--no-leading-addr', co).splitlines():
    m = re.match(r'^[0-9a-f]* ?<(.+)>:$', line)
    if m:
      cur = code.setdefault(m.group(1), [])
    elif cur is not None and line.strip():
      cur.append(re.sub(r'\s*//.*$', '', line).strip())    # the comment holds the address and the encoding
  return kernels, resources, code


def main(a_dir, b_dir):
  bad = 0
  for name in OBJECTS:
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
      ka, ra, ca = read_code_object(code_object(os.path.join(a_dir, name), ta))
      kb, rb, cb = read_code_object(code_object(os.path.join(b_dir, name), tb))
    findings = ['kernel only in A: ' + n for n in sorted(ka - kb)] + ['kernel only in B: ' + n for n in sorted(kb - ka)]
    findings += ['function only in A: ' + n for n in sorted(set(ca) - set(cb))]
    findings += ['function only in B: ' + n for n in sorted(set(cb) - set(ca))]
    for n in sorted(ka & kb):
      if n not in ra or n not in rb or None in ra[n] or n not in ca:
        findings.append('no metadata or no code found (parser out of date?): ' + n)
      elif ra[n] != rb[n]:
        findings.append('resources differ: %s: %s vs %s' % (n, ra[n], rb[n]))
    findings += ['instructions differ: ' + n for n in sorted(set(ca) & set(cb)) if ca[n] != cb[n]]
    for f in findings:
      print('  %s: %s' % (name, f))
    print('%-16s %4d kernels in A, %4d in B, %9d instructions compared: %s'
          % (name, len(ka), len(kb), sum(len(v) for v in ca.values()),
             'identical' if not findings else '%d DIFFERENCES' % len(findings)))
    bad += len(findings)
  print('code objects: ' + ('IDENTICAL per kernel (symbols, resources, instructions)' if bad == 0 else '%d differences' % bad))
  return 1 if bad else 0


if __name__ == '__main__':
  if len(sys.argv) != 3:
    sys.exit(__doc__)
  sys.exit(main(sys.argv[1], sys.argv[2]))
