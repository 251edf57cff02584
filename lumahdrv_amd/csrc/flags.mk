# Compiler and flags of the device code (its own file so that lumahdrv_amd.capi.kernel_source_sha covers the flags but not
# the rules for tools and examples in the Makefile).
#   -ffp-contract=off : the reference arithmetic is un-contracted fp32 (see luma_device.hpp); fma()
#                       appears only where written explicitly.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
FLAGS   := --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -Wall -Wno-unused-function $(EXTRA)
# Per-translation-unit additions (the Makefile appends $(FLAGS_<unit>) to the unit's compile line).
#   lumahip_encode: LLVM's "max-ilp" machine-scheduling strategy.  Same-box A/B of the whole library built either way (round 6,
#   profiles/r06_sched_ab.txt): the HBM-bound encode kernels 1.6 - 1.8 % faster per launch, the decode kernels 0.9 % SLOWER, the
#   VALU-bound YCbCr kernels unchanged -- so it is the encode unit's only.  ("iterative-ilp" crashes this compiler on these units.)
FLAGS_lumahip_encode := -mllvm -amdgpu-sched-strategy=max-ilp
FLAGS_lumahip_encode_f16 := $(FLAGS_lumahip_encode)
#   lumahip_transcode: the default strategy.  Its kernels are neither the HBM-bound encode kernels max-ilp helped nor measured
#   either way yet: no A/B, no flag.
FLAGS_lumahip_transcode :=
#   lumahip_transcode_half: the transcode unit's -- k_transcode_half is k_transcode with four source units folded into one target unit.
FLAGS_lumahip_transcode_half := $(FLAGS_lumahip_transcode)
#   lumahip_transcode_quarter: the same -- k_transcode_quarter is k_transcode_half with sixteen source units folded into one target unit.
FLAGS_lumahip_transcode_quarter := $(FLAGS_lumahip_transcode)
#   lumahip_transcode_distortion: the transcode unit's -- its kernels are k_transcode's front end with the measuring consumer.
FLAGS_lumahip_transcode_distortion := $(FLAGS_lumahip_transcode)
#   lumahip_transcode_distortion_map: the same -- k_transcode_distortion_map is k_transcode_distortion with the accumulation in space.
FLAGS_lumahip_transcode_distortion_map := $(FLAGS_lumahip_transcode)
#   lumahip_transcode_moments_map: the same -- k_transcode_moments_map is k_transcode_distortion_map with another consumer.
FLAGS_lumahip_transcode_moments_map := $(FLAGS_lumahip_transcode)
#   lumahip_transcode_half_distortion / _map: the same -- their kernels are k_transcode_half's front end with the measuring consumers.
FLAGS_lumahip_transcode_half_distortion := $(FLAGS_lumahip_transcode)
FLAGS_lumahip_transcode_half_distortion_map := $(FLAGS_lumahip_transcode)
#   lumahip_distortion / _f16: the encode units' strategy -- k_distortion is k_encode up to the codes, with the stores replaced by
#   integer accumulation.  Not measured either way yet.
FLAGS_lumahip_distortion := $(FLAGS_lumahip_encode)
FLAGS_lumahip_distortion_f16 := $(FLAGS_lumahip_encode)
#   lumahip_distortion_map / _f16: the same -- k_distortion_map is k_distortion with the accumulation in space.
FLAGS_lumahip_distortion_map := $(FLAGS_lumahip_encode)
FLAGS_lumahip_distortion_map_f16 := $(FLAGS_lumahip_encode)
#   lumahip_moments_map / _f16: the same -- k_moments_map is k_distortion_map with another consumer.
FLAGS_lumahip_moments_map := $(FLAGS_lumahip_encode)
FLAGS_lumahip_moments_map_f16 := $(FLAGS_lumahip_encode)
#   lumahip_planes_measure: the decode unit's (the default strategy) -- its kernels are the decode kernels' plane loads and integer
#   accumulation, with none of the encode arithmetic max-ilp was measured on.
FLAGS_lumahip_planes_measure :=
#   lumahip_light_level: the decode unit's (the default strategy) -- its kernels are loads, the decode arithmetic of the plane-fed
#   family and integer accumulation; not measured either way.
FLAGS_lumahip_light_level :=
