"""CPU-only tests of the resident bf16 dataset image (include/codae_hip.h, codae_set_dataset_image): the header / binding agreement
on the new entries, and who registers an image - HipEmbeddingTrainer, for the bf16 engine only, unless dataset_image=False or
CODAE_NO_DATASET_IMAGE says otherwise.  The trainer is built on a recording stand-in for DaeEngine: no device is needed to
see what it asks of its engine."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_the_new_entries_with_abi_11():
    from codae import hip
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    assert int(re.search(r"#define CODAE_ABI_VERSION (\d+)", header).group(1)) == 11 == hip.ABI_VERSION      # new entries only
    assert int(re.search(r"#define CODAE_N_STRUCTS (\d+)", header).group(1)) == 7
    for name in ("codae_set_dataset_image", "codae_corrupt_batch_image"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        assert name in hip.PROTOTYPES and len(hip.PROTOTYPES[name][1]) == m.group(1).count(",") + 1, name
    assert re.search(r"int codae_set_dataset_image\(codae_handle h, const float\* data, const void\* image_bf16, int64_t n_rows, int32_t io\);",
                     header)
    assert re.search(r"int codae_corrupt_batch_image\(const codae_batch\* batch, const void\* image_bf16, const uint8_t\* present, "
                     r"int32_t n_slots, void\* out,\s+int64_t out_ld, void\* stream\);", header)
    # the contract a caller has to know: the image is not refreshed behind their back
    assert "registers the image again" in header
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("codae_set_dataset_image", "codae_corrupt_batch_image", "CODAE_NO_DATASET_IMAGE", "CODAE_NO_FOLDED_BIAS_FINISH"):
        assert word in integration, word


def test_the_switches_are_read_with_the_other_toggles():
    """both new switches live in EnvToggles and are read in env_reload, where every CODAE_* switch is read: never on a launch path"""
    common = open(os.path.join(ROOT, "mui-deepautoencoder_amd", "csrc", "codae_common.h")).read()
    engine = open(os.path.join(ROOT, "mui-deepautoencoder_amd", "csrc", "engine.hip")).read()
    toggles = common[common.index("struct EnvToggles"):common.index("const EnvToggles& env();")]
    reload_body = engine[engine.index("void env_reload()"):engine.index("const EnvToggles& env()")]
    for field, var in (("no_dataset_image", "CODAE_NO_DATASET_IMAGE"), ("no_folded_bias_finish", "CODAE_NO_FOLDED_BIAS_FINISH")):
        assert field in toggles, field
        assert 'getenv("%s")' % var in reload_body, var
        assert engine.count('"%s"' % var) == 1, var


class _Engine:
    """what HipEmbeddingTrainer.__init__ touches of a DaeEngine when no optional setting is given"""
    made = []

    def __init__(self, schedule, max_batch, precision, device, activation=None):
        from codae.hip.engine import precision_code
        self.precision = precision_code(precision)
        self.image_of = []
        _Engine.made.append(self)

    def set_dataset_image(self, data):
        self.image_of.append(data)


@pytest.fixture
def trainer(monkeypatch):
    import codae.hip.engine as E
    from codae.train import HipEmbeddingTrainer
    monkeypatch.setattr(E, "DaeEngine", _Engine)
    monkeypatch.delenv("CODAE_NO_DATASET_IMAGE", raising=False)
    _Engine.made.clear()

    def make(precision, **kw):
        data = torch.arange(48, dtype=torch.float32).reshape(6, 8)
        return HipEmbeddingTrainer([(8, 8, False)], data, None, None, 1e-3, 0.0, max_batch=4, precision=precision, device="cpu", **kw)
    return make


def test_the_trainer_registers_an_image_of_its_own_dataset_for_bf16_only(trainer):
    from codae.train import HipEmbeddingTrainer
    assert inspect.signature(HipEmbeddingTrainer.__init__).parameters["dataset_image"].default is True
    tr = trainer("bf16")
    assert len(tr.engine.image_of) == 1 and tr.engine.image_of[0] is tr.data      # the very tensor the batches are made from
    tr.refresh_dataset_image()                                                     # (after rewriting tr.data in place)
    assert len(tr.engine.image_of) == 2 and tr.engine.image_of[1] is tr.data
    for precision in ("f32", "parity"):
        tr = trainer(precision)
        assert tr.engine.image_of == []
        tr.refresh_dataset_image()
        assert tr.engine.image_of == []


def test_the_keyword_and_the_env_switch_keep_the_old_path(trainer, monkeypatch):
    tr = trainer("bf16", dataset_image=False)
    assert tr.dataset_image is False and tr.engine.image_of == []
    monkeypatch.setenv("CODAE_NO_DATASET_IMAGE", "1")
    tr = trainer("bf16")
    assert tr.dataset_image is False and tr.engine.image_of == []
    tr.refresh_dataset_image()
    assert tr.engine.image_of == []
    monkeypatch.delenv("CODAE_NO_DATASET_IMAGE")
    tr = trainer("bf16")
    assert tr.dataset_image is True and len(tr.engine.image_of) == 1


def test_the_engine_casts_and_registers_nothing_for_fp32():
    """DaeEngine.set_dataset_image on an fp32 engine clears the registration and allocates no image (read off the method: building
    an engine needs a device)"""
    from codae.hip.engine import DaeEngine
    src = inspect.getsource(DaeEngine.set_dataset_image)
    head = src[:src.index("torch.empty")]
    assert "self.precision != PREC_BF16" in head and "codae_set_dataset_image(self._h, None, None, 0, 0)" in head and "return None" in head
