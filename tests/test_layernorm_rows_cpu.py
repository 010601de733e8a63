"""ViT-Ti/16 and ViT-S/16: the classes build by name from their recipe configs."""
import json
from pathlib import Path

import pytest

from pytorch_distributed_template_amd import models
from pytorch_distributed_template_amd.config import ConfigParser

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("tag,cls,params,rate", [("ti16", models.ViT_Ti_16, 5717416, 0.0),
                                                 ("s16", models.ViT_S_16, 22050664, 0.1)])
def test_small_vits_build_from_their_configs(tag, cls, params, rate, tmp_path):
    cfg = json.loads((ROOT / "config" / f"vit_{tag}_bf16_packed_mix_ema_dp_re.json").read_text())
    base = json.loads((ROOT / "config" / "vit_b16_fp8_packed_mix_ema_dp_re.json").read_text())
    assert cfg["arch"]["args"] == dict(num_classes=1000, fp8=False, drop_path_rate=rate)
    assert all(cfg[k] == base[k] for k in base if k not in ("name", "arch"))
    cfg["trainer"]["save_dir"] = str(tmp_path / "ck")
    m = ConfigParser(cfg, run_id=tag).init_obj("arch", models)
    assert type(m) is cls and not m.fp8 and m.drop_path_rates[-1] == pytest.approx(rate)
    assert sum(p.numel() for p in m.parameters()) == params
