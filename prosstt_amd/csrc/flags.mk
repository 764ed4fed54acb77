# The hipcc flags of every HIP library of the package (included by Makefile, stats/Makefile, embed/Makefile, knn/Makefile, graph/Makefile and layout/Makefile; host/ uses
# g++ and flags of its own).
#   -ffp-contract=off  the sampler's definition (PRNB-5) spells out every fma; nothing else may fuse
#   -fno-slp-vectorize packed binary32 instructions take two issue slots on gfx950 and cost moves to pair their operands
#   -mllvm -amdgpu-sched-strategy=max-ilp  the scheduler orders for instruction-level parallelism, not register pressure (the
#                      stream kernel keeps its 5 blocks per CU: tests/test_kernel_isa.py): -0.9 % of the call, bit-exact
#   IEEE sqrt/divide   hipcc's default (-fhip-fp32-correctly-rounded-divide-sqrt); never -ffast-math
# tests/test_kernel_isa.py, tests/test_count_summary_isa.py, tests/test_embed_isa.py, tests/test_knn_isa.py, tests/test_graph_isa.py and tests/test_layout_isa.py compile the sources themselves and repeat
# these flags on purpose: whoever changes one here changes it there too.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
FLAGS   := --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize \
           -mllvm -amdgpu-sched-strategy=max-ilp -fPIC -shared -fvisibility=hidden \
           -Wall -Wextra -Wno-unused-parameter
