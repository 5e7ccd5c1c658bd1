# Build of the product library (HIP, gfx950) and the CPU oracle (test infrastructure).
#   make            -> orb_slam3_comments_ghr_amd/liborbslam3_amd.so + oracle/liboracle.so
HIPCC ?= hipcc
ARCH ?= gfx950
PKG = orb_slam3_comments_ghr_amd
CSRC = $(PKG)/csrc
LIB = $(PKG)/liborbslam3_amd.so
OBJDIR = build/obj
HIPFLAGS = --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wall -Wno-unused-function
# bit-exact float geometry in the matcher and BowVector sums: no FMA contraction in those units
EXACT = -ffp-contract=off
# make POSE_PROF=1: phase cycle counters in k_pose_opt (tools/pose_prof.py)
ifdef POSE_PROF
HIPFLAGS += -DOSG_POSE_PROF
endif
# make SR_PROF=1: k_schur_rows_c's per-workgroup timeline (tools/sr_prof.py)
ifdef SR_PROF
HIPFLAGS += -DOSG_SR_PROF
endif
# make MLPNP_PROF=1: k_mlpnp_eval's per-stage clock stamps in place of the per-hypothesis poses (tools/mlpnp_prof.py)
ifdef MLPNP_PROF
HIPFLAGS += -DOSG_MLPNP_PROF
endif
HDRS = include/osg.h include/osg_ba.h include/osg_imu.h $(CSRC)/osg_internal.h
# the small dense routines (host and device) and the SO(3) functions built on them
LINALG_HDRS = $(CSRC)/small_linalg.h $(CSRC)/osg_hd.h
SO3_HDRS = $(CSRC)/so3_common.h $(LINALG_HDRS)
# the RANSAC solvers' shared device helpers and host batch scaffolding
RANSAC_HDRS = $(CSRC)/ransac_common.h $(CSRC)/batch_io.h $(CSRC)/glibc_math.h $(LINALG_HDRS)
# the pointer-binding packer and the launch sequence of the entry points built on it
PACKED_HDRS = $(CSRC)/match_common.h $(CSRC)/packed_launch.h

OBJS = $(OBJDIR)/runtime.o $(OBJDIR)/hamming.o $(OBJDIR)/hamming_mfma.o $(OBJDIR)/match.o $(OBJDIR)/pose.o $(OBJDIR)/poseinertial.o $(OBJDIR)/inertialopt.o $(OBJDIR)/localinertialba.o $(OBJDIR)/preintegrate.o $(OBJDIR)/sim3opt.o $(OBJDIR)/sim3ransac.o $(OBJDIR)/mlpnp.o $(OBJDIR)/twoview.o $(OBJDIR)/essgraph.o $(OBJDIR)/ba.o $(OBJDIR)/dbow.o $(OBJDIR)/kfdb.o $(OBJDIR)/fuse.o $(OBJDIR)/triang.o $(OBJDIR)/newpoints.o $(OBJDIR)/frustum.o $(OBJDIR)/desc.o $(OBJDIR)/sim3.o $(OBJDIR)/init.o $(OBJDIR)/stereo.o $(OBJDIR)/orb.o $(OBJDIR)/fast.o $(OBJDIR)/pyramid.o

WALL_BENCH = tools/adapter_wall_bench

all: $(LIB) oracle $(WALL_BENCH)

$(OBJDIR):
	mkdir -p $(OBJDIR)

$(OBJDIR)/runtime.o: $(CSRC)/runtime.hip $(HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJDIR)/hamming.o: $(CSRC)/hamming.hip $(HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/hamming_mfma.o: $(CSRC)/hamming_mfma.hip $(HDRS) $(CSRC)/top2_key.h $(CSRC)/top2_ring.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJDIR)/match.o: $(CSRC)/match.hip $(HDRS) $(CSRC)/match_common.h $(CSRC)/frustum_common.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/pose.o: $(CSRC)/pose.hip $(HDRS) $(CSRC)/ba_common.h $(CSRC)/exact_math.h $(CSRC)/glibc_math.h $(CSRC)/match_common.h $(LINALG_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/poseinertial.o: $(CSRC)/poseinertial.hip $(HDRS) $(CSRC)/ba_common.h $(CSRC)/poseinertial_common.h $(SO3_HDRS) $(CSRC)/exact_math.h $(RANSAC_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/inertialopt.o: $(CSRC)/inertialopt.hip $(HDRS) $(CSRC)/ba_common.h $(CSRC)/inertialopt_common.h $(CSRC)/poseinertial_common.h $(SO3_HDRS) $(CSRC)/exact_math.h $(CSRC)/batch_io.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/localinertialba.o: $(CSRC)/localinertialba.hip $(HDRS) $(CSRC)/ba_common.h $(CSRC)/inertialba_edges.h $(CSRC)/localinertialba_common.h $(CSRC)/poseinertial_common.h $(SO3_HDRS) $(CSRC)/exact_math.h $(CSRC)/glibc_math.h $(CSRC)/batch_io.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/preintegrate.o: $(CSRC)/preintegrate.hip $(HDRS) $(CSRC)/imu_common.h $(SO3_HDRS) $(CSRC)/batch_io.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/sim3opt.o: $(CSRC)/sim3opt.hip $(HDRS) $(CSRC)/ba_common.h $(CSRC)/sim3_common.h $(CSRC)/exact_math.h $(CSRC)/glibc_math.h $(CSRC)/batch_io.h $(LINALG_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/sim3ransac.o: $(CSRC)/sim3ransac.hip $(HDRS) $(CSRC)/sim3ransac_select.h $(RANSAC_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/mlpnp.o: $(CSRC)/mlpnp.hip $(HDRS) $(CSRC)/mlpnp_select.h $(RANSAC_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/twoview.o: $(CSRC)/twoview.hip $(HDRS) $(CSRC)/twoview_select.h $(RANSAC_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/essgraph.o: $(CSRC)/essgraph.hip $(HDRS) $(CSRC)/sim3_common.h $(CSRC)/exact_math.h $(CSRC)/essgraph4_common.h $(SO3_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/ba.o: $(CSRC)/ba.hip $(HDRS) $(CSRC)/ba_common.h $(CSRC)/exact_math.h $(CSRC)/glibc_math.h $(CSRC)/match_common.h $(CSRC)/osg_hd.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OBJDIR)/dbow.o: $(CSRC)/dbow.hip $(HDRS) include/osg_dbow.h $(CSRC)/match_common.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@
$(OBJDIR)/kfdb.o: $(CSRC)/kfdb.hip $(HDRS) include/osg_dbow.h $(CSRC)/kfdb_select.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@

$(OBJDIR)/fuse.o: $(CSRC)/fuse.hip $(HDRS) $(PACKED_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@

$(OBJDIR)/triang.o: $(CSRC)/triang.hip $(HDRS) $(PACKED_HDRS) $(CSRC)/kb8_epipolar.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@

$(OBJDIR)/newpoints.o: $(CSRC)/newpoints.hip $(HDRS) $(CSRC)/kb8_epipolar.h $(RANSAC_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@

$(OBJDIR)/frustum.o: $(CSRC)/frustum.hip $(HDRS) $(CSRC)/frustum_common.h $(RANSAC_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@

$(OBJDIR)/desc.o: $(CSRC)/desc.hip $(HDRS) $(CSRC)/match_common.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJDIR)/sim3.o: $(CSRC)/sim3.hip $(HDRS) $(PACKED_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@

$(OBJDIR)/init.o: $(CSRC)/init.hip $(HDRS) $(PACKED_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@

$(OBJDIR)/stereo.o: $(CSRC)/stereo.hip $(HDRS) $(PACKED_HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@

$(OBJDIR)/orb.o: $(CSRC)/orb.hip $(HDRS) $(CSRC)/match_common.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@

$(OBJDIR)/fast.o: $(CSRC)/fast.hip $(HDRS) $(CSRC)/match_common.h $(CSRC)/octree.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@

$(OBJDIR)/pyramid.o: $(CSRC)/pyramid.hip $(HDRS) $(CSRC)/match_common.h | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXACT) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf build $(LIB)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean

# the C++ adapter wall-rate bench (bench.py's wall_cpp_adapter_frames_per_s): host code over the
# library and the HIP runtime (device-resident pyramid levels for the stereo workload)
$(WALL_BENCH): tools/adapter_wall_bench.cpp adapters/orbslam3/osg_orbslam3.h tests/adapter/driver_common.h tests/adapter/mock_orbslam3.h include/osg.h include/osg_ba.h include/osg_dbow.h include/osg_imu.h $(LIB)
	g++ -std=c++17 -O2 -Wall -Werror -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude $< -o $@ -L$(PKG) -lorbslam3_amd -L/opt/rocm/lib -lamdhip64 '-Wl,-rpath,$$ORIGIN/../$(PKG)' -Wl,-rpath,/opt/rocm/lib -pthread
