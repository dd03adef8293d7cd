"""What a refine call launches (clustertracking_amd/csrc/refine_plan.h) without a
device: tests/native/refine_plan_main.cpp, a program of its own, built with the address and
undefined-behaviour sanitizers and run as a child process.  Over every combination of

* throughput flag, 2D / 3D, lowpass, a window of <= 600 / > 600 pixels, tail_absorb 0 / 5 / default;
* pairs 0, 1, 63, 64, 2048, 2049; 3-feature (NT 1) and 5-feature (NT 2) clusters 0, 1, tail_absorb,
  tail_absorb + 1; singles 0, 1, 9; a large and a too-large cluster present or not

(tables with a bin of 8192 or 8193 clusters: singles, large and too-large cluster all absent or all
present; and, for problems that cannot have a tail launch, no pairs or 2049) it exits non-zero unless

a. the flags, the tail segments and the launch list equal a restatement of the rules with literal
   numbers, field by field;
b. for every non-empty bin and every device-side count of close clusters in {0, 1, count - 1, count},
   the entries that the bin's launches and its tail segment take (kargs.h: KArgs::split*, TailArgs)
   partition the bin: no cluster fitted twice, none left out;
c. bin_begin is the prefix sum of bin_count, the order is a permutation that holds each bin
   contiguously, and a block bin runs by descending feature count, stably.
"""
import os
import subprocess

import _cases

SRC = os.path.join(_cases.ROOT, 'tests', 'native', 'refine_plan_main.cpp')
INCLUDES = [os.path.join(_cases.ROOT, 'clustertracking_amd', 'csrc'), os.path.join(_cases.ROOT, 'include')]


def test_refine_plan_decision(tmp_path):
    exe = tmp_path / 'refine_plan_main'
    # (the sanitizers' runtimes are linked into the program itself: it runs in whatever
    # environment the suite runs in, with nothing added to it and nothing taken from it)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-static-libasan', '-static-libubsan',
                           '-Wall', '-Werror'] + [f'-I{d}' for d in INCLUDES] + [SRC, '-o', str(exe)],
                          timeout=300)
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = run.stdout.decode(errors='replace')
    assert run.returncode == 0, out[-4000:]
    assert 'refine_plan: ok' in out
