"""What the compiler recorded about the kernels of the built libctrefine.so: the metadata note of the
gfx950 code objects, for the test_*_resources.py files (CPU only).  A helper module like _cases.py;
every file keeps its own kernel list and its own assertions."""
import os
import re
import shutil
import subprocess

LLVM_BIN = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


class Unavailable(AssertionError):
    """no library, no LLVM tools or no readable fat binary: nothing about a kernel"""


def _tool(name):
    p = os.path.join(LLVM_BIN, name)
    return p if os.path.exists(p) else shutil.which(name)


def metadata(prefix, tmp):
    """{mangled kernel name: its metadata fields} of every kernel whose name holds ``prefix``; ``tmp``: a
    pathlib directory for the unbundled code objects"""
    from clustertracking_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        raise Unavailable('libctrefine.so is not built')
    objcopy, bundler, readelf = _tool('llvm-objcopy'), _tool('clang-offload-bundler'), _tool('llvm-readelf')
    if not (objcopy and bundler and readelf):
        raise Unavailable('llvm-objcopy / clang-offload-bundler / llvm-readelf not found')
    fatbin = str(tmp / 'fatbin')
    subprocess.check_call([objcopy, '--dump-section', '.hip_fatbin=' + fatbin, _lib.LIB_PATH, str(tmp / 'lib.so')])
    # one offload bundle per translation unit, back to back in the section
    data = open(fatbin, 'rb').read()
    starts = [m.start() for m in re.finditer(re.escape(b'__CLANG_OFFLOAD_BUNDLE__'), data)]
    if not starts:
        raise Unavailable('the fat binary holds no uncompressed offload bundles')
    out = {}
    for j, (s, e) in enumerate(zip(starts, starts[1:] + [len(data)])):
        if prefix.encode() not in data[s:e]:
            continue
        bundle, co = str(tmp / ('bundle%d' % j)), str(tmp / ('gfx950_%d.co' % j))
        with open(bundle, 'wb') as f:
            f.write(data[s:e])
        subprocess.check_call([bundler, '--type=o', '--unbundle', '--targets=' + TARGET, '--input=' + bundle, '--output=' + co])
        notes = subprocess.check_output([readelf, '--notes', co], text=True)
        # the amdhsa.kernels list of the metadata note: one "- .agpr_count: ..." block per kernel
        for block in re.split(r'\n\s+- \.agpr_count:', notes)[1:]:
            fields = dict(re.findall(r'^\s*(\.[a-z_]+):\s+(\S+)\s*$', '.agpr_count:' + block, re.M))
            if '.name' in fields and prefix in fields['.name']:
                out[fields['.name']] = fields
    return out
