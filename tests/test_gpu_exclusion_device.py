"""Clade exclusion with the keys on the device (MCQ_DEVICE_PTRS of mcq_ws_set_exclusion and mcq_ws_set_query_clades), and under
MCQ_QUIRK_SEQ_DROP with keys that exclude: both against OracleDb.reduce_query on the Python-filtered match lists, as
test_gpu_exclusion.py defines exclusion."""
import numpy as np
import pytest

from test_gpu_exclusion import GENUS, SPECIES, _db, _expected, _same, _world

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,P", [("mini", 4), ("noanc", 2)])
def test_table_and_keys_as_device_pointers(tag, P):
    import torch
    w = _world(tag, P)
    eng = w["eng"]
    dev = torch.device("cuda", 0)
    ws = eng.Workspace(_db(w), w["nq"], len(w["bases"]))
    for rank in (SPECIES, GENUS):
        d_tgt = torch.from_numpy(np.ascontiguousarray(w["tgt"][rank]).view(np.int32).copy()).to(dev)     # (the u32 bit patterns)
        d_key = torch.from_numpy(np.ascontiguousarray(w["qkey"][rank]).view(np.int32).copy()).to(dev)
        torch.cuda.synchronize(dev)
        ws.set_exclusion(None, device_ptr=d_tgt.data_ptr(), n_targets=len(w["tgt"][rank]))
        d_tgt.fill_(7)                                                # the table was copied by the call
        torch.cuda.synchronize(dev)
        for max_cand in (1, 4):
            ws.set_query_clades(None, device_ptr=d_key.data_ptr(), n_queries=w["nq"])
            got = ws.query_host(w["bases"], w["seq_off"], True, max_cand=max_cand, emulate_ranks=P)
            _same(got, _expected(w, rank, max_cand, P), (tag, P, "device keys", rank, max_cand))
        with pytest.raises(eng.McqError) as e:                        # consumed by one call, like a host array
            ws.query_host(w["bases"], w["seq_off"], True, max_cand=2, emulate_ranks=P)
        assert e.value.code == eng.MCQ_E_ARG


@pytest.mark.parametrize("tag,P", [("mini", 4), ("tie", 2), ("noanc", 2)])
def test_exclusion_under_the_sequence_drop_quirk(tag, P):
    """MCQ_QUIRK_SEQ_DROP acts on the merge of the emulated ranks' lists, after the excluded targets are gone: the oracle's
    reduce with the quirk on, on the filtered match lists"""
    w = _world(tag, P)
    eng, fx = w["eng"], w["fx"]
    ws = eng.Workspace(_db(w), w["nq"], len(w["bases"]))
    for rank in (SPECIES, GENUS):
        tgt, qk = w["tgt"][rank], w["qkey"][rank]
        ws.set_exclusion(tgt)
        for max_cand in (fx.maxcand, 1):
            cands = np.zeros((w["nq"], max_cand, 4), np.uint32)
            ncand = np.zeros(w["nq"], np.uint32)
            for q in range(w["nq"]):
                m = w["matches"][q]
                if qk[q] != eng.MCQ_CLADE_KEEP_ALL:
                    m = m[tgt[(m >> np.uint64(32)).astype(np.int64)] != qk[q]]
                cands[q], ncand[q] = w["odb"].reduce_query(m, len(fx.r1[q]) + len(fx.r2[q]), max_cand=max_cand, emulate_ranks=P, quirk_seq_drop=1)
            ws.set_query_clades(qk)
            got = ws.query_host(w["bases"], w["seq_off"], True, max_cand=max_cand, emulate_ranks=P, flags=eng.MCQ_QUIRK_SEQ_DROP)
            _same(got, (cands, ncand), (tag, P, "quirk", rank, max_cand))
