"""frontdoor.read_tim_tsv / write_tim_tsv: the reference's four-field TSV of the front-door features (path_id, then base64 of one
float32 row per modality; tab-separated, no header).  CPU only."""
import base64
import csv

import numpy as np
import torch

from vln_goat_amd import frontdoor

FIELDS = ['path_id', 'txt_feats', 'vp_feats', 'gmap_feats']


def _tables(n=5, h=24, seed=3):
    rs = np.random.RandomState(seed)
    t = [rs.standard_normal((n, h)).astype(np.float32) for _ in range(3)]
    t[0][0, :4] = [0.0, -0.0, np.float32(1e-42), np.float32(3.4e38)]      # signed zero, a denormal, near the float32 maximum
    return t


def test_fieldnames_are_the_references():
    assert frontdoor.TIM_TSV_FIELDNAMES == FIELDS


def test_write_then_read_round_trips_bit_exactly(tmp_path):
    txt, vp, gmap = _tables()
    path = str(tmp_path / 'r2r_cfp_features.tsv')
    ids = [7001, 12, 533, 533, 90210]
    frontdoor.write_tim_tsv(path, ids, torch.from_numpy(txt), vp, torch.from_numpy(gmap))       # tensors and arrays alike
    got = frontdoor.read_tim_tsv(path)
    for a, b in zip(got, (txt, vp, gmap)):
        assert a.dtype == np.float32 and a.shape == b.shape
        assert a.tobytes() == b.tobytes()
    assert frontdoor.read_tim_tsv_ids(path) == [str(i) for i in ids]
    d = frontdoor.read_tim_tsv(path, return_dict=True)
    assert sorted(d) == sorted(FIELDS[1:])
    assert len(d['vp_feats']) == 5 and d['vp_feats'][3].tobytes() == vp[3].tobytes()
    lines = open(path).read().splitlines()
    assert len(lines) == 5 and all(len(ln.split('\t')) == 4 for ln in lines)                    # no header, four fields


def test_reads_lines_written_the_way_the_reference_agent_writes_them(tmp_path):
    """The writer loop of the reference's extract_cfp_features: rows are CPU tensors taken out of the batch outputs,
    base64.b64encode(np.array(row)) -> str, csv.DictWriter with a tab delimiter and no header."""
    txt, vp, gmap = _tables(n=3, h=16, seed=9)
    rows = [list(torch.from_numpy(t)) for t in (txt, vp, gmap)]
    path = str(tmp_path / 'ref_style.tsv')
    with open(path, 'wt') as f:
        w = csv.DictWriter(f, delimiter='\t', fieldnames=FIELDS)
        for i in range(3):
            w.writerow({'path_id': 100 + i,
                        'txt_feats': str(base64.b64encode(np.array(rows[0][i].numpy())), 'utf-8'),
                        'vp_feats': str(base64.b64encode(np.array(rows[1][i].numpy())), 'utf-8'),
                        'gmap_feats': str(base64.b64encode(np.array(rows[2][i].numpy())), 'utf-8')})
    got = frontdoor.read_tim_tsv(path)
    for a, b in zip(got, (txt, vp, gmap)):
        assert a.tobytes() == b.tobytes()
    # and the other direction: the same tables through write_tim_tsv give the same bytes on disk
    ours = str(tmp_path / 'ours.tsv')
    frontdoor.write_tim_tsv(ours, [100, 101, 102], txt, vp, gmap)
    assert open(ours, 'rb').read() == open(path, 'rb').read()


def test_save_features_layout(tmp_path):
    """The reference's save_features (frontdoor_update_features.tsv): n_clusters lines, path_id 0."""
    k = 6
    txt, vp, gmap = _tables(n=k, h=8, seed=4)
    path = str(tmp_path / 'frontdoor_update_features.tsv')
    frontdoor.write_tim_tsv(path, 0, txt, vp, gmap)
    assert frontdoor.read_tim_tsv_ids(path) == ['0'] * k
    d = frontdoor.read_tim_tsv(path, return_dict=True)
    assert all(len(d[f]) == k for f in FIELDS[1:])
    assert np.array(d['gmap_feats']).tobytes() == gmap.tobytes()


def test_write_rejects_mismatched_tables(tmp_path):
    import pytest
    txt, vp, gmap = _tables()
    with pytest.raises(ValueError):
        frontdoor.write_tim_tsv(str(tmp_path / 'x.tsv'), [1, 2], txt, vp, gmap)
    with pytest.raises(ValueError):
        frontdoor.write_tim_tsv(str(tmp_path / 'x.tsv'), 0, txt, vp[:3], gmap)
