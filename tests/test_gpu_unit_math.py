"""The unit-domain forms of the sampling math on the device (rt_device.h dm_sincos_nonneg / dm_acos_unit / dm_cbrt_unit /
random_in_unit_sphere_unit, called by shade_hit in every path kernel): exhaustively against the general device functions and the CPU
oracle, and through two small renders with the default launch plan whose frames and ray counts must be the oracle's."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unit_forms_equal_the_general_forms_and_the_oracle_on_every_input(tmp_path, orc):
    """tests/native/unit_math_exhaustive.hip: all 2^23 values of random::<f32>() through sin / cos(theta), acos, sin / cos(phi) and cbrt in
    both forms on the GPU, and the composed sampler on 2^22 generator states; every float equal to the general form's and to liboracle's."""
    exe = str(tmp_path / "unit_math_exhaustive")
    odir = os.path.join(ROOT, "oracle")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I", os.path.join(ROOT, "tiny-raytracer_amd", "csrc"),
                    "-I", odir, "-o", exe, os.path.join(ROOT, "tests", "native", "unit_math_exhaustive.hip"), "-L", odir, "-loracle",
                    "-Wl,-rpath," + odir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]


@pytest.mark.parametrize("name", ["cornell", "dummy_spheres"])
def test_default_plan_renders_equal_the_oracle(trt, orc, name):
    """Cornell 64x64 (Lambertian lanes, 8 spp, depth 50) and the reference's 5-sphere world 64x48 (metal and dielectric lanes): default
    backend and plan, frame bit for bit and the ray count."""
    desc = trt.scenes.cornell(64, 64) if name == "cornell" else trt.scenes.dummy_spheres("renderer", 64, 48)
    world, cam = trt.world_from_description(desc)
    renderer = trt.Renderer(8, 1, 50, False, desc["background"], seed=1)
    gpu = renderer.render(cam, world, collect_stats=False).data
    rays = renderer.last_stats["rays"]
    oworld, ocam = orc.world_from_description(desc)
    cpu, stats = orc.render(oworld, ocam, 8, 50, desc["background"], seed=1, nthreads=8)
    differ = int((np.ascontiguousarray(gpu, np.float32).view(np.uint32) != np.ascontiguousarray(cpu, np.float32).view(np.uint32)).sum())
    print(f"{name}: {differ} of {gpu.size} values differ; rays {rays} (oracle {stats['rays']})")
    assert differ == 0
    assert rays == stats["rays"]
