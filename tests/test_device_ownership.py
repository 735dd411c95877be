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


OWNED = re.compile(r'(?:DevBuf|PinnedBuf)<[^>]*>\s+([^;(]*);')
PLANNED = re.compile(r'unique_ptr<[^;]*>\s+(\w+);')
# what this context keeps itself (the shard's data, the globals, the outputs): every stage of an evaluation owns its buffers in a state struct, every
# feature that only runs on demand in a plan of its own
GP_CTX_MAX_BUFFERS = 24


def _owned(body):
    """The DevBuf / PinnedBuf members a struct body declares, every declarator of each declaration."""
    return [re.match(r'\s*(\w+)', d).group(1) for decl in OWNED.findall(body) for d in decl.split(',')]


def _owner_structs():
    """gp_ctx and every struct of csrc/ that owns device memory (a DevBuf or PinnedBuf member): the plans and their groups."""
    owners = {}
    for f in sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h'))):
        code = _code(f)
        for m in re.finditer(r'\bstruct\s+(\w+)\s*\{', code):
            body = _body(code[m.start():], m.group(0))
            if m.group(1) == 'gp_ctx' or OWNED.search(body):
                assert m.group(1) not in owners, 'two owner structs named ' + m.group(1)
                owners[m.group(1)] = body
    return owners


def test_gp_destroy_names_no_buffer():
    owners = _owner_structs()
    ctx = owners['gp_ctx']
    owned = [n for body in owners.values() for n in _owned(body) + PLANNED.findall(body)]
    assert len(owned) > 60 and 'Kaug' in owned and 'p1plan' in owned and 'h_out' in owned, owned
    # the plans of the on-demand families (regime B, predict, infer), each held by the context through one owner
    for plan, member, field in (('BPlan', 'LET', 'bplan'), ('PredPlan', 'P1', 'pred'), ('InferPlan', 'Gf', 'infer')):
        assert plan in owners and member in _owned(owners[plan]), (plan, member)
        assert field in PLANNED.findall(ctx), field
    # the state of the stages of an evaluation, each struct a single member of the context
    for state, member, field in (('GsState', 'Linv', 'gstep'), ('P2State', 'HZp', 'p2')):
        assert state in owners and member in _owned(owners[state]), (state, member)
        assert member not in _owned(ctx), member
        assert re.search(r'\b%s\s+%s;' % (state, field), ctx), field
    # every pointer-typed field of the context and of the plans is an owner (the RCCL communicator and the HIP events are not memory)
    for name, body in owners.items():
        raw = [m for m in re.findall(r'^\s*[\w:]+\s*\*\s*(\w+)', body, re.M) if not (name == 'gp_ctx' and m == 'comm')]
        assert not raw, 'raw pointer fields in %s: %s' % (name, raw)
    body = _body(_code(os.path.join(CSRC, 'api.hip')), 'extern "C" int gp_destroy(gp_ctx* c)')
    named = sorted(set(re.findall(r'c->(\w+)', body)) & set(owned))
    assert not named, 'gp_destroy frees buffers by name: %s' % named
    assert 'delete c' in body


def test_gp_ctx_holds_no_feature_buffers():
    n = len(_owned(_owner_structs()['gp_ctx']))
    assert n <= GP_CTX_MAX_BUFFERS, 'gp_ctx owns %d device buffers (at most %d): give a new feature a plan of its own' % (n, GP_CTX_MAX_BUFFERS)


def test_alloc_fail_after_is_a_known_option():
    from gparml_amd import _lib
    lib = _lib.load()
    assert lib.gp_debug_set_option(b'alloc_fail_after', 0) == _lib.GP_OK
    assert lib.gp_debug_set_option(b'no_such_option', 1) == _lib.GP_ERR_BAD_ARG
    assert b'alloc_fail_after' in lib.gp_last_error(None)
