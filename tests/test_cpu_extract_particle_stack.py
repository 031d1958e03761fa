"""`topaz extract --particle-stack` without a GPU: the planner half both entry points share, the refusals that come before
anything is loaded, and the arithmetic that places every rank's particles in the one output file."""
import io
import os
import socket

import numpy as np
import pandas as pd
import pytest
import torch.multiprocessing as mp

from conftest import GOLDEN

PS = os.path.join(GOLDEN, 'particle_stack')
CLI = os.path.join(GOLDEN, 'cli')
PICKS = os.path.join(CLI, 'extract_picks.txt')


def _records_of(table_path, threshold, image_root):
    """the pick table restated as the in-memory records `extract` holds, and the first micrograph's (mz, cella, cellb)"""
    from topaz_amd import mrc
    from topaz_amd.utils.picks import Record
    t = pd.read_csv(table_path, sep='\t')
    if 'score' in t:
        t = t.loc[t['score'] >= threshold]
    records, first = [], None
    for name, g in t.groupby('image_name'):
        if first is None:
            with open(os.path.join(image_root, str(name) + '.mrc'), 'rb') as f:
                h = mrc.parse_header(f.read(1024))
            first = (h.nz, (h.xlen, h.ylen, h.zlen), (h.alpha, h.beta, h.gamma))
        records.append(Record(str(name) + '.mrc', g[['x_coord', 'y_coord']].values.astype(np.int32),
                              g['score'].values if 'score' in g else None))
    return records, first


def _no_score_table(tmp_path):
    t = pd.read_csv(PICKS, sep='\t').drop(columns='score')
    p = tmp_path / 'no_score.txt'
    t.to_csv(p, sep='\t', index=False)
    return str(p)


@pytest.mark.parametrize('case', ['score', 'threshold', 'no_score', 'frames_metadata', 'resize_metadata', 'resize_odd'])
def test_in_memory_planner_equals_the_file_planner(case, tmp_path):
    from topaz_amd.utils.picks import plan_from_records, plan_particle_stack
    table, root, size, resize, threshold, meta = PICKS, CLI, 32, -1, -np.inf, None
    if case == 'threshold':
        size, threshold = 33, -5.0
    elif case == 'no_score':
        table = _no_score_table(tmp_path)
    elif case == 'frames_metadata':
        table, root, size, meta = os.path.join(PS, 'picks3.txt'), PS, 9, os.path.join(PS, 'meta3.star')
    elif case == 'resize_metadata':
        resize, meta = 16, os.path.join(PS, 'meta_ab.star')
    elif case == 'resize_odd':
        resize = 15
    out = '/somewhere/stack32.mrcs'
    plan = plan_particle_stack(table, out, threshold, size, resize, root, '.mrc', meta, log=io.StringIO())
    records, (mz, cella, cellb) = _records_of(table, threshold, root)
    header, star_path, star = plan_from_records(records, out, size, size if resize < 0 else resize, mz, cella, cellb, meta)
    assert header == plan.header and len(header) == 1024
    assert star == plan.star and star_path == plan.star_path == '/somewhere/stack32.star'
    assert ('AutopickFigureOfMerit' in star) == (case != 'no_score')
    assert sum(len(r.xy) for r in records) == plan.n
    if case == 'score':                                   # ... which is the reference's own output
        assert header == open(os.path.join(PS, 'stack32.mrcs'), 'rb').read(1024)
        assert star == open(os.path.join(PS, 'stack32.star')).read()


def test_star_scores_are_what_particle_stack_reads_back_from_the_table():
    """the table holds the float64 digits of the float32 scores; the STAR holds what pandas' parser makes of that text -- which
    is not always that float64 value, so the in-memory path has to go through the same text and the same parser"""
    from topaz_amd.utils.picks import Record, plan_from_records, scores_as_read_back
    t = pd.read_csv(PICKS, sep='\t')
    s32 = t.score.values.astype(np.float32)                  # the scores `extract` held when it wrote the table
    text = [ln.split('\t')[3] for ln in open(PICKS).read().splitlines()[1:]]
    assert text == [repr(float(v)) for v in s32]             # (the table does hold those digits)
    xy = t[['x_coord', 'y_coord']].values
    got = scores_as_read_back(xy, s32)
    assert got.dtype == np.float64 and np.array_equal(got, t.score.values)
    off = int((got != s32.astype(np.float64)).sum())
    print(off, 'of', len(got), 'scores are not the float64 value of the float32 score')
    assert np.abs(got - s32.astype(np.float64)).max() <= 2 ** -50 * np.abs(got).max()     # (an ulp, where at all)
    assert len(scores_as_read_back(np.zeros((0, 2), np.int32), np.zeros(0, np.float32))) == 0
    rec = [Record('mic.mrc', xy, got)]
    star = plan_from_records(rec, 'o.mrcs', 8, 8, 1, (1, 1, 1), (0, 0, 0), None)[2]
    rows = [ln.split('\t') for ln in star.splitlines() if ln.startswith('mic.mrc')]
    assert [r[3] for r in rows] == [repr(float(v)) for v in t.score.values]


STACK = ['--particle-stack', 'out.mrcs']
REFUSED = [
    (STACK, 'particle-size'),                                                   # no box size
    (STACK + ['--particle-size', '0'], 'particle-size'),
    (STACK + ['--particle-size', '32', '--particle-resize', '0'], 'particle-resize'),
    (STACK + ['--particle-size', '32', '--particle-resize', '33'], 'particle-resize'),
    (STACK + ['--particle-size', '32', '--dims', '3'], 'dims 2'),
    (STACK + ['--particle-size', '32', '-m', 'none'], 'model'),
    (STACK + ['--particle-size', '32', '--targets', 'targets.txt'], 'targets'),
    (STACK + ['--particle-size', '32', '--only-validate'], 'only-validate'),
]
BAD_LISTS = [
    (['a.mrc', 'b.tiff'], r'\.mrc'),                                            # not an MRC file
    (['a.mrc', 'b.png'], r'\.mrc'),
    (['b.mrc', 'a.mrc'], 'sorted'),
    (['x/a.mrc', 'y/a.mrc'], 'sorted'),                                         # a duplicate name
    (['mic_10.mrc', 'mic_9.mrc', 'mic_11.mrc'], 'sorted'),                      # plain string order, not numeric
]


def _nothing_may_load(monkeypatch):
    from topaz_amd import extract as ex
    from topaz_amd import runtime as rt

    def boom(*a, **k):
        raise AssertionError('nothing may be loaded before the arguments are checked')

    for name in ('load_model', 'Scorer', 'ImageFeed', 'load_image'):
        monkeypatch.setattr(ex, name, boom)
    monkeypatch.setattr(rt, 'get_context', boom)
    for v in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize('extra,match', REFUSED)
def test_bad_arguments_raise_before_anything_is_loaded(monkeypatch, tmp_path, extra, match):
    from topaz_amd import extract as ex
    from topaz_amd.commands import extract as cmd
    _nothing_may_load(monkeypatch)
    monkeypatch.chdir(tmp_path)
    args = cmd.add_arguments().parse_args(['-r', '8', '-o', 'picks.txt', 'a.mrc', 'b.mrc'] + extra)
    with pytest.raises(ValueError, match=match):
        cmd.main(args)
    # the library entry refuses the same combinations
    with pytest.raises(ValueError, match=match):
        ex.extract_particles(args.paths, args.model, 0, 1, -6.0, 8, 0, args.targets, 5, 100, 5, None, 0, args.only_validate,
                             'picks.txt', False, '', 'coord', 1, 1, dims=args.dims, particle_stack=args.particle_stack,
                             particle_size=args.particle_size, particle_resize=args.particle_resize)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize('paths,match', BAD_LISTS)
def test_bad_input_lists_raise_before_anything_is_loaded(monkeypatch, tmp_path, paths, match):
    from topaz_amd.commands import extract as cmd
    _nothing_may_load(monkeypatch)
    monkeypatch.chdir(tmp_path)
    args = cmd.add_arguments().parse_args(['-r', '8', '-o', 'picks.txt'] + STACK + ['--particle-size', '32'] + paths)
    with pytest.raises(ValueError, match=match):
        cmd.main(args)
    assert os.listdir(tmp_path) == []
    # without the flag the same list is none of this feature's business: it gets as far as loading the model
    args = cmd.add_arguments().parse_args(['-r', '8', '-o', 'picks.txt'] + paths)
    with pytest.raises(AssertionError, match='nothing may be loaded'):
        cmd.main(args)


def test_a_sorted_list_passes_the_checks(monkeypatch, tmp_path):
    from topaz_amd.commands import extract as cmd
    from topaz_amd.utils.picks import check_particle_stack_inputs
    check_particle_stack_inputs([])
    check_particle_stack_inputs(['z/only.mrc'])
    check_particle_stack_inputs(sorted(f'raw/mic_{i}.mrc' for i in range(30)))     # what a shell glob hands over
    check_particle_stack_inputs(['b/Mic.mrc', 'a/mic.mrc', 'a/mic_1.mrc'])          # names decide, not directories
    _nothing_may_load(monkeypatch)
    monkeypatch.chdir(tmp_path)
    args = cmd.add_arguments().parse_args(['-r', '8', '-o', 'picks.txt'] + STACK + ['--particle-size', '32', '--particle-resize',
                                                                                  '16', 'a.mrc', 'b.mrc'])
    with pytest.raises(AssertionError, match='nothing may be loaded'):               # (past every refusal: the model is next)
        cmd.main(args)


def test_flags_parse_with_the_defaults_of_particle_stack():
    from topaz_amd.commands import extract
    from topaz_amd.commands._spec import PARTICLE_STACK, build_parser
    a = extract.add_arguments().parse_args(['-r', '8', 'a.mrc'])
    p = build_parser(PARTICLE_STACK, '').parse_args(['picks.txt'])
    assert (a.particle_stack, a.particle_size, a.particle_resize, a.particle_threshold, a.particle_metadata) == \
        (None, p.size, p.resize, p.threshold, p.metadata) == (None, None, -1, -np.inf, None)
    b = extract.add_arguments().parse_args(['-r', '8', '--particle-stack', 'o.mrcs', '--particle-size', '64', '--particle-resize',
                                            '32', '--particle-threshold', '-1.5', '--particle-metadata', 'm.star', 'a.mrc'])
    assert (b.particle_stack, b.particle_size, b.particle_resize, b.particle_threshold, b.particle_metadata) == \
        ('o.mrcs', 64, 32, -1.5, 'm.star')


def test_particle_stack_takes_gpus_under_the_topaz_entry_point(monkeypatch):
    from topaz_amd import main as tmain
    from topaz_amd import parallel
    seen = {}
    monkeypatch.setattr(parallel, 'launch_local_ranks', lambda n, cmd, env=None, **kw: seen.update(n=n, cmd=list(cmd)) or 0)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    argv = ['particle_stack', 'picks.txt', '--size', '32', '-o', 'o.mrcs', '--gpus', '2']
    assert tmain.main(argv) == 0
    assert seen['n'] == 2 and seen['cmd'][-len(argv):] == argv


def _prefix_sums(counts):
    return [int(v) for v in np.concatenate([[0], np.cumsum(counts)[:-1]])]


@pytest.mark.parametrize('world', [1, 2, 3])
def test_offsets_are_the_prefix_sums_of_the_counts_in_input_order(world):
    from topaz_amd.utils.picks import particle_offset
    counts = [5, 0, 7, 3, 0, 0, 11, 2, 9, 4]                    # ten micrographs: the last round of world 3 is ragged
    if world == 2:
        counts = counts[:9]                                     # ... and of world 2
    want = _prefix_sums(counts)
    got = {}
    for rank in range(world):
        base = 0
        for r0 in range(0, len(counts), world):
            in_round = counts[r0:r0 + world]
            in_round += [0] * (world - len(in_round))           # ranks without an image contribute 0
            first, base = particle_offset(base, in_round, rank)
            if r0 + rank < len(counts):
                got[r0 + rank] = first
        assert base == sum(counts)                              # every rank ends up knowing the stack length
    assert [got[i] for i in range(len(counts))] == want


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


COUNTS = [4, 0, 6, 1, 3]                                        # five micrographs on two ranks: rank 1 sits out the last round


def _claim_worker(rank, world, port, out_path, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), TOPAZ_AMD_NO_AFFINITY='1')
    import torch
    from topaz_amd import parallel
    from topaz_amd.utils.picks import ExtractStack
    ranks = parallel.init_from_env('gloo')
    stack = ExtractStack(out_path, 32, -1, -np.inf, None, ranks)
    mine = parallel.shard_indices(len(COUNTS), rank, world)
    firsts = [stack.claim(COUNTS[i]) for i in mine]
    for _ in range(len(mine), -(-len(COUNTS) // world)):
        stack.skip_round()
    q.put((rank, list(zip(mine, firsts)), stack.base))
    torch.distributed.destroy_process_group()


def test_two_ranks_agree_on_the_offsets_gloo(tmp_path):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_claim_worker, args=(r, 2, port, str(tmp_path / 'o.mrcs'), q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    got, bases = {}, []
    for _ in range(2):
        rank, pairs, base = q.get(timeout=5)
        got.update(dict(pairs))
        bases.append(base)
    assert [got[i] for i in range(len(COUNTS))] == _prefix_sums(COUNTS) == [0, 4, 4, 10, 11]
    assert bases == [sum(COUNTS)] * 2
