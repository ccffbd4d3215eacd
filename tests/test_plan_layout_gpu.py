"""A live handle runs the plan the host-only planner lays out: for the bench's and the aortic pipeline's headline cases the handle's
kernel_names() / kernel_configs() equal engine.plan_layout(..., cus = this device's compute units), and its workspace is the
layout's activation maps.  (tests/test_plan_layout.py holds the full matrix, on the CPU, against the recorded plans.)"""
import pytest

pytestmark = pytest.mark.gpu

CASES = [('FCN_sa', 'fp32', 64, 192, 208), ('FCN_sa', 'bf16', 64, 192, 208), ('UNet_ao', 'fp32', 100, 256, 256), ('UNet_ao', 'bf16', 100, 256, 256),
         ('UNet-LSTM_ao', 'fp32', 50, 256, 256), ('UNet-LSTM_ao', 'bf16', 50, 256, 256), ('Temporal-UNet_ao', 'fp32', 18, 64, 96)]


@pytest.mark.parametrize('model,prec,n,H,W', CASES)
def test_live_handle_runs_the_laid_out_plan(model, prec, n, H, W):
    import torch
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS[model]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = engine.plan_layout(arch, prec, n, H, W, cus=cus)
    with engine.Engine(arch, synthetic_params(arch, 1234)) as eng:
        eng.set_precision(prec)
        eng.reserve(n, H, W)
        assert eng.kernel_names() == [o['name'] for o in plan['ops']]
        assert eng.kernel_configs() == [o['cfg'] if o['kind'] in ('conv', 'tconv') else -1 for o in plan['ops']]
        assert eng.scratch_bytes() == 4 * n * sum(a['per_image'] for a in plan['acts'])
