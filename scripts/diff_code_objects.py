#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code objects of two builds of jpd-se_amd/csrc (a change of the host layer must leave
them alone; it is what stands in for "kernel speed unchanged").

  python scripts/diff_code_objects.py [--match-by-content] CSRC_DIR_A CSRC_DIR_B

CSRC_DIR_x: a csrc directory after `make` (it holds conv_gemm.o, conv_gemm.dev.o, norm.o, norm.dev.o, elementwise.o,
binarize.o, metrics.o, msssim_loss.o, entropy.o, semantics.o, code_rate.o, sem_loss.o, code_cost.o, vq.o, vq_coder.o,
vq_plane.o, vq_cost.o, vq_bottleneck.o, vq_fit.o, vq_ec.o, vq_residual.o, vq_res_ec.o, vq_res_rate.o).  Per object file the gfx950 code object is taken out of the .hip_fatbin section (llvm-objcopy + clang-offload-bundler), then compared PER SYMBOL -- host code that
instantiates kernels in another order may reorder them inside the object:
  * the set of kernels (the .kd symbols),
  * the resources of each (vgpr / sgpr / agpr count, LDS and scratch size, kernarg size: the metadata note),
  * the instruction stream of each function (llvm-objdump -d, addresses and encodings stripped).
--match-by-content: for a change that renames kernels (a shorter template parameter list changes the mangled name).  Kernels
present on one side only are paired by exact equality of (resources, instruction list) and compared under B's name; each pair
is printed as `renamed:<TAB>old<TAB>new` (mangled, then demangled: the table scripts/compare_kernel_traces.py --rename reads).
Bodies that are identical to each other pair in any order; a kernel without a partner stays "only in A / only in B".
Exit status 0 when nothing differs, 1 otherwise."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM_BIN', '/opt/rocm/llvm/bin')
OBJECTS = ['conv_gemm.o', 'conv_gemm.dev.o', 'norm.o', 'norm.dev.o', 'elementwise.o', 'binarize.o', 'metrics.o', 'msssim_loss.o',
           'entropy.o', 'semantics.o', 'code_rate.o', 'sem_loss.o', 'code_cost.o', 'vq.o', 'vq_coder.o', 'vq_plane.o', 'vq_cost.o', 'vq_bottleneck.o',
           'vq_fit.o', 'vq_ec.o', 'vq_residual.o', 'vq_res_ec.o', 'vq_res_rate.o']
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


def read_code_object(co, pcrel=False):
  """(kernel names, {kernel: resources}, {function symbol: [instructions]}); pcrel: the pc-relative address of a device variable
  (s_getpc_b64 + s_add_u32 literal) is written as the variable's name and the alignment filler behind a function is dropped:
  both move with the layout of the linked object, which a renamed kernel changes"""
  kernels, data = set(), {}
  for line in tool('llvm-readelf', '-s', '--wide', co).splitlines():
    f = line.split()
    if len(f) >= 8 and f[3] == 'OBJECT' and f[7].endswith('.kd'):
      kernels.add(f[7][:-3])
    elif len(f) >= 8 and f[3] == 'OBJECT':
      data[int(f[1], 16)] = f[7]
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
      m = pcrel and cur and cur[-1].startswith('s_getpc_b64') and re.match(r'^\s*(s_add_u32 .*, )0x([0-9a-f]+)\s*// ([0-9A-F]+):', line)
      if m and int(m.group(3), 16) + int(m.group(2), 16) in data:
        line = m.group(1) + data[int(m.group(3), 16) + int(m.group(2), 16)]
      cur.append(re.sub(r'\s*//.*$', '', line).strip())    # the comment holds the address and the encoding
  for insns in code.values() if pcrel else ():
    while insns and insns[-1] in ('s_nop 0', 's_code_end', '...'):      # alignment filler behind the function: layout, not code
      insns.pop()
  return kernels, resources, code


def pair_by_content(ka, ra, ca, kb, rb, cb):
  """renames A's one-sided kernels to the B kernel of equal (resources, instructions); a reference to the own symbol is neutral"""
  def groups(names, r, c):
    g = {}
    for n in sorted(names):
      g.setdefault((r.get(n), tuple(i.replace(n, '<self>') for i in c.get(n, ()))), []).append(n)
    return g
  ga, gb = groups(ka - kb, ra, ca), groups(kb - ka, rb, cb)
  for key, olds in ga.items():
    news = gb.get(key, [])
    if len(news) != len(olds):            # no partner, or more candidates on one side than the other: left unpaired
      continue
    for old, new in zip(olds, news):
      print('renamed:\t%s\t%s' % (old, new))
      print('renamed:\t%s\t%s' % tuple(subprocess.run(['c++filt', old, new], check=True, capture_output=True, text=True).stdout.split('\n')[:2]))
      ka.remove(old), ka.add(new)
      ra[new] = ra.pop(old)
      ca[new] = [i.replace(old, new) for i in ca.pop(old)]


def main(a_dir, b_dir, by_content=False):
  bad = 0
  for name in OBJECTS:
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
      ka, ra, ca = read_code_object(code_object(os.path.join(a_dir, name), ta), by_content)
      kb, rb, cb = read_code_object(code_object(os.path.join(b_dir, name), tb), by_content)
    if by_content:
      pair_by_content(ka, ra, ca, kb, rb, cb)
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
  args = [a for a in sys.argv[1:] if a != '--match-by-content']
  if len(args) != 2:
    sys.exit(__doc__)
  sys.exit(main(args[0], args[1], len(args) != len(sys.argv) - 1))
