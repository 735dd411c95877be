"""Device memory has one owner (gparml_amd/csrc/devbuf.h, gp::DevBuf): no other source allocates or frees GPU memory, and a context's buffers are
freed by deleting the context, not by a list in gp_destroy that has to be kept in step with gp_ctx."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, 'gparml_amd', 'csrc')
OWNER = 'devbuf.h'
RAW_ALLOC = re.compile(r'\bhip(Host)?(Malloc|Free)')
# developer timing builds only: a static scratch buffer that lives until the process ends
TIMING_BLOCK = re.compile(r'#ifdef (GPARML_GEN8_TIMING|GPARML_TILE_TIMING)\b.*?#endif', re.S)


def _code(path):
    """The source with its comments removed (string literals kept)."""
    src = open(path).read()
    return re.sub(r'//[^\n]*|/\*.*?\*/', '', src, flags=re.S)


def _body(src, head):
    i = src.index(head)
    j = src.index('{', i)
    depth = 0
    for k in range(j, len(src)):
        depth += {'{': 1, '}': -1}.get(src[k], 0)
        if depth == 0:
            return src[j:k + 1]
    raise AssertionError('unbalanced braces after ' + head)


def test_only_the_owner_allocates_device_memory():
    files = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))
    assert os.path.join(CSRC, OWNER) in files
    offenders = []
    for f in files:
        if os.path.basename(f) == OWNER:
            continue
        code = TIMING_BLOCK.sub('', _code(f))
        for m in RAW_ALLOC.finditer(code):
            offenders.append('%s:%d: %s' % (os.path.basename(f), code.count('\n', 0, m.start()) + 1, m.group(0)))
    assert not offenders, 'raw allocation outside %s: %s' % (OWNER, offenders)
    assert RAW_ALLOC.search(_code(os.path.join(CSRC, OWNER)))


def test_gp_destroy_names_no_buffer():
    ctx = _body(_code(os.path.join(CSRC, 'gp_common.h')), 'struct gp_ctx {')
    owned = re.findall(r'(?:DevBuf|PinnedBuf)<[^>]*>\s+(\w+)', ctx) + re.findall(r'unique_ptr<[^;]*>\s+(\w+);', ctx)
    assert len(owned) > 60 and 'Kaug' in owned and 'p1plan' in owned and 'h_out' in owned, owned
    # every pointer-typed field of the context is an owner (the RCCL communicator and the HIP events are not memory)
    raw = [m for m in re.findall(r'^\s*[\w:]+\s*\*\s*(\w+)', ctx, re.M) if m != 'comm']
    assert not raw, 'raw pointer fields in gp_ctx: %s' % raw
    body = _body(_code(os.path.join(CSRC, 'api.hip')), 'extern "C" int gp_destroy(gp_ctx* c)')
    named = sorted(set(re.findall(r'c->(\w+)', body)) & set(owned))
    assert not named, 'gp_destroy frees buffers by name: %s' % named
    assert 'delete c' in body


def test_alloc_fail_after_is_a_known_option():
    from gparml_amd import _lib
    lib = _lib.load()
    assert lib.gp_debug_set_option(b'alloc_fail_after', 0) == _lib.GP_OK
    assert lib.gp_debug_set_option(b'no_such_option', 1) == _lib.GP_ERR_BAD_ARG
    assert b'alloc_fail_after' in lib.gp_last_error(None)
