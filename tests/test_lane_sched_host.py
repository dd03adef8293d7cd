"""The placement policy of the lanes (clustertracking_amd/csrc/lane_sched.h) without a
device: tests/native/lane_sched_main.cpp, a program of its own, built with the address and
undefined-behaviour sanitizers and run as a child process.  It exits non-zero unless

1. every multiset of at most 7 chain durations out of {1, 2, 3, 5, 8, 13} on 1..4 lanes is placed
   within the LPT bound (4/3 - 1/(3 L)) of the optimum (brute force);
2. one lane takes every chain;
3. the finish chain is on the lane of the longest bin chain;
4. with completions in every order that respects lane order the loads never go negative, return
   to exactly zero, and tickets retire from the front of a lane only;
5. a launch's estimate is the static guess before its first reading and the last valid reading
   after it (0, negative and non-finite readings are ignored);
6. the lane limit restricts placement to the first n lanes and 0 restores all.
"""
import os
import subprocess

import _cases

SRC = os.path.join(_cases.ROOT, 'tests', 'native', 'lane_sched_main.cpp')
INCLUDE = os.path.join(_cases.ROOT, 'clustertracking_amd', 'csrc')


def test_lane_sched_policy(tmp_path):
    exe = tmp_path / 'lane_sched_main'
    # (the sanitizers' runtimes are linked into the program itself: it runs in whatever
    # environment the suite runs in, with nothing added to it and nothing taken from it)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-static-libasan', '-static-libubsan',
                           '-Wall', '-Werror', '-I', INCLUDE, SRC, '-o', str(exe)],
                          timeout=300)
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = run.stdout.decode(errors='replace')
    assert run.returncode == 0, out[-4000:]
    assert 'lane_sched: ok' in out
