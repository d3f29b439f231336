// AppFusion on the MI355X library (apps/src/app_fusion.cpp:64-200 of the reference), written against include/intrinsic3d_hip.h only.
//
//   app_fusion -s <path>/sensor.yml -f <path>/fusion.yml [--device N]
//
// As in the reference the working directory becomes the directory of sensor.yml and ./fusion is created; the frames (keyframes only when
// fusion.yml names a keyframes file) are fused into a TSDF volume on the device, corrected, cleaned, saved as `output_sdf`, and the
// marching-cubes mesh of the volume is saved as `output_mesh`.
//
// Opt-in, not in the reference: `track_frames: "1"` registers every fused frame after the first against the volume fused so far
// (i3d_fusion_track) and integrates it at the registered pose; `output_tracked_poses: "<file>"` writes the trajectory in Sensor::savePoses layout.
// `track_mode: "sdf"` registers on the volume's field instead (i3d_fusion_track_sdf); `track_mode: "sdf_rgbd"` adds the volume's fused
// colour (i3d_fusion_track_sdf_rgbd) with the optional `track_photo_weight`.
// `repose_passes: "N"` (only together with track_frames) runs N leave-one-out passes over the fused frames after the sequence: every frame
// but the first is taken out of the volume (i3d_fusion_deintegrate), registered against the rest by the tracker of track_mode from its tracked pose, and integrated
// again at the result; the frames are read again through the sensor handle.
// `resume_volume: "file.tsdf"` starts from a saved volume (i3d_fusion_load) instead of an empty one; the configured voxel_size must be the
// file's, bit for bit.  `checkpoint_every: "N"` with `checkpoint_volume: "file.tsdf"` saves the open volume's records (i3d_fusion_snapshot + i3d_fusion_save) after
// every N-th fused frame.  `correct_iterations: "N"` sets the sweeps of correctSDF before saving (the reference's 10 when absent).
#include "../include/intrinsic3d_hip.h"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <sys/stat.h>
#include <unistd.h>

namespace {
std::string yaml(const std::string& file, const char* key, const char* fallback = "") {
    char buf[4096];
    return i3d_yaml_get(file.c_str(), key, buf, sizeof(buf)) == I3D_OK ? std::string(buf) : std::string(fallback);
}
float yamlf(const std::string& file, const char* key) { return (float)std::atof(yaml(file, key, "0").c_str()); }
std::string absolute(const std::string& p) { char buf[PATH_MAX]; return realpath(p.c_str(), buf) ? std::string(buf) : p; }

// world -> camera angle-axis | t -> 4x4 world -> camera (row-major), Rodrigues as i3d_sensor_set_pose_vec6
void mat_from_vec6(const double* p, double* m) {
    const double th = std::sqrt(p[0] * p[0] + (p[1] * p[1] + p[2] * p[2]));
    double k[3] = {0, 0, 0}; if (th > 0.0) { k[0] = p[0] / th; k[1] = p[1] / th; k[2] = p[2] / th; }
    const double c = std::cos(th), sn = std::sin(th), v = 1.0 - c;
    const double r[16] = {c + k[0] * k[0] * v, k[0] * k[1] * v - k[2] * sn, k[0] * k[2] * v + k[1] * sn, p[3],
                          k[1] * k[0] * v + k[2] * sn, c + k[1] * k[1] * v, k[1] * k[2] * v - k[0] * sn, p[4],
                          k[2] * k[0] * v - k[1] * sn, k[2] * k[1] * v + k[0] * sn, c + k[2] * k[2] * v, p[5], 0, 0, 0, 1};
    for (int i = 0; i < 16; ++i) m[i] = r[i];
}
void rigid_inverse(const double* m, double* o) {           // [R t; 0 1]^-1 = [R^T -R^T t; 0 1]
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) o[4 * a + b] = m[4 * b + a];
        o[4 * a + 3] = -(m[a] * m[3] + m[4 + a] * m[7] + m[8 + a] * m[11]);
    }
    o[12] = o[13] = o[14] = 0.0; o[15] = 1.0;
}
// The frame's luminance at the depth camera's geometry: the colour pixel of depth pixel (u, v) by the lookup of the integration at any
// depth - the two cameras share a centre - round_trunc(((u - cx_d) / fx_d) fx_c + cx_c) in float, then 0.114 b + 0.587 g + 0.299 r of the pixel / 255 in
// float; NaN (no photometric sample) where the pixel falls outside the colour image
void luminance_at_depth_geometry(const uint8_t* bgr, const int32_t* cwh, const float* ci, const int32_t* dwh, const float* di, float* lum) {
    const float k = (float)(1.0 / 255.0);
    for (int v = 0; v < dwh[1]; ++v) {
        const int py = (int)((((float)v - di[3]) / di[1]) * ci[1] + ci[3] + 0.5f);
        for (int u = 0; u < dwh[0]; ++u) {
            const int px = (int)((((float)u - di[2]) / di[0]) * ci[0] + ci[2] + 0.5f);
            float out = std::nanf("");
            if (px >= 0 && py >= 0 && px < cwh[0] && py < cwh[1]) {
                const uint8_t* c = &bgr[((size_t)py * cwh[0] + px) * 3];
                const float b = (float)c[0] * k, g = (float)c[1] * k, r = (float)c[2] * k;
                out = (b * 0.114f + g * 0.587f) + r * 0.299f;
            }
            lum[(size_t)v * dwh[0] + u] = out;
        }
    }
}
void mat_mul(const double* x, const double* y, double* o) {
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) { double s = 0.0; for (int k = 0; k < 4; ++k) s += x[4 * a + k] * y[4 * k + b]; o[4 * a + b] = s; }
}
}  // namespace

int main(int argc, char* argv[]) {
    std::string sensor_cfg, fusion_cfg; int device = 0;
    for (int i = 1; i < argc; ++i) {
        std::string arg = argv[i], val; const size_t eq = arg.find('=');
        if (eq != std::string::npos) { val = arg.substr(eq + 1); arg = arg.substr(0, eq); } else if (i + 1 < argc) val = argv[++i];
        if (arg == "-s" || arg == "--sensor") sensor_cfg = val;
        else if (arg == "-f" || arg == "--fusion") fusion_cfg = val;
        else if (arg == "--device") device = std::atoi(val.c_str());
        else { std::fprintf(stderr, "usage: %s -s <sensor.yml> -f <fusion.yml> [--device N]\n", argv[0]); return 2; }
    }
    if (sensor_cfg.empty() || fusion_cfg.empty()) { std::fprintf(stderr, "usage: %s -s <sensor.yml> -f <fusion.yml> [--device N]\n", argv[0]); return 2; }
    sensor_cfg = absolute(sensor_cfg); fusion_cfg = absolute(fusion_cfg);
    const std::string dir = sensor_cfg.substr(0, sensor_cfg.find_last_of('/'));
    if (chdir(dir.c_str()) != 0) { std::fprintf(stderr, "cannot change the working directory to %s\n", dir.c_str()); return 1; }
    mkdir("./fusion", 0755);

    i3d_sensor* sensor = nullptr;
    float depth_min = 0.0f, depth_max = 0.0f;
    int rc = i3d_sensor_open_yaml(sensor_cfg.c_str(), &sensor, &depth_min, &depth_max);                    // Sensor::create(sensor_cfg)
    int32_t num_frames = 0, num_loaded = 0, cwh[2] = {0, 0}, dwh[2] = {0, 0}; float ci[4], di[4];
    if (rc == I3D_OK) i3d_sensor_info(sensor, &num_frames, &num_loaded, cwh, dwh, ci, di);
    if (rc != I3D_OK || num_loaded == 0) { std::fprintf(stderr, "RGB-D sensor could not be initialized!\n"); return 1; }
    std::printf("%d filenames loaded.\n", num_frames);

    // keyframes (optional): fuse only the selected frames (app_fusion.cpp:112-120,145-149)
    std::vector<uint8_t> is_kf; bool use_kf = false;
    const std::string kf_file = yaml(fusion_cfg, "keyframes");
    if (!kf_file.empty()) {
        use_kf = true; int32_t window = 0; uint64_t n = 0;
        if (i3d_keyframes_load(kf_file.c_str(), &window, 0, nullptr, nullptr, &n) == I3D_OK) { is_kf.resize(n); i3d_keyframes_load(kf_file.c_str(), &window, n, nullptr, is_kf.data(), &n); }
        else std::fprintf(stderr, "Could not load keyframes ...\n");
    }

    const float voxel_size = yamlf(fusion_cfg, "voxel_size");
    const float clip[6] = {yamlf(fusion_cfg, "clip_x0"), yamlf(fusion_cfg, "clip_x1"), yamlf(fusion_cfg, "clip_y0"), yamlf(fusion_cfg, "clip_y1"), yamlf(fusion_cfg, "clip_z0"),
                           yamlf(fusion_cfg, "clip_z1")};
    i3d_fusion* vol = nullptr;
    // opt-in "resume_volume": the volume comes from a saved .tsdf (i3d_fusion_load) and the frames are fused on top of it
    const std::string resume_file = yaml(fusion_cfg, "resume_volume");
    if (!resume_file.empty()) {
        float file_vs = 0.0f;
        if (i3d_tsdf_read_header(resume_file.c_str(), &file_vs, nullptr, nullptr, nullptr, nullptr) != I3D_OK) {
            std::fprintf(stderr, "resume_volume: cannot read %s\n", resume_file.c_str()); return 1;
        }
        if (std::memcmp(&file_vs, &voxel_size, sizeof(float)) != 0) {
            std::fprintf(stderr, "resume_volume: the file's voxel size %.9g is not the configured voxel_size %.9g\n", (double)file_vs, (double)voxel_size); return 1;
        }
        std::printf("Resuming the volume of %s ...\n", resume_file.c_str());
        rc = i3d_fusion_load(device, resume_file.c_str(), depth_min, depth_max, clip, &vol);
    } else rc = i3d_fusion_create(device, voxel_size, depth_min, depth_max, clip, 1u << 22, &vol);
    if (rc != I3D_OK) { std::fprintf(stderr, rc == I3D_ERR_NO_DEVICE ? "no HIP device %d\n" : "Could not create voxel grid! (%d)\n", rc == I3D_ERR_NO_DEVICE ? device : rc); return 1; }
    // opt-in "checkpoint_every: N" + "checkpoint_volume: file": the open volume's records (i3d_fusion_snapshot) saved after every N-th fused frame
    const int checkpoint_every = std::atoi(yaml(fusion_cfg, "checkpoint_every", "0").c_str());
    const std::string checkpoint_file = yaml(fusion_cfg, "checkpoint_volume");
    if (checkpoint_every < 0 || (checkpoint_every > 0) != !checkpoint_file.empty()) {
        std::fprintf(stderr, "checkpoint_every (a count > 0) and checkpoint_volume (a file) go together\n"); return 1;
    }
    // opt-in "prune_every: N": after every N-th fused frame the voxels of weight <= prune_min_weight (default 0: the weightless ones) and, with
    // "prune_max_sdf_voxels" > 0, those further than that many voxel sizes from the surface leave the volume and its table shrinks (i3d_fusion_prune, section 38)
    const int prune_every = std::atoi(yaml(fusion_cfg, "prune_every", "0").c_str());
    const float prune_min_weight = (float)std::atof(yaml(fusion_cfg, "prune_min_weight", "0").c_str());
    const float prune_max_sdf = (float)std::atof(yaml(fusion_cfg, "prune_max_sdf_voxels", "0").c_str()) * voxel_size;
    if (prune_every < 0) { std::fprintf(stderr, "prune_every must be a count >= 0 (0: never)\n"); return 1; }
    // opt-in "components_min_voxels: N": after the last frame and before the volume is finished, the connected components of weighted voxels with fewer than N
    // voxels - floaters - leave the volume and its table shrinks (one i3d_fusion_prune_components(0, 0, N, 0, 1), section 39)
    const long long components_min_voxels = std::atoll(yaml(fusion_cfg, "components_min_voxels", "0").c_str());
    if (components_min_voxels < 0) { std::fprintf(stderr, "components_min_voxels must be a count >= 0 (0: off)\n"); return 1; }
    // opt-in "correct_iterations": the sweeps of correctSDF before saving (the reference's 10 when absent)
    const int correct_iterations = std::atoi(yaml(fusion_cfg, "correct_iterations", "10").c_str());
    if (correct_iterations < 0) { std::fprintf(stderr, "correct_iterations must be >= 0\n"); return 1; }
    std::printf("SDF volume info:\n   voxel size: %g\n   truncation: %g\n   integration depth min: %g\n   integration depth max: %g\n", (double)voxel_size, (double)(voxel_size * 5.0f),
                (double)depth_min, (double)depth_max);

    const int erode = std::atoi(yaml(fusion_cfg, "discont_window_size", "0").c_str());
    // opt-in frame-to-model tracking: the first fused frame keeps its sensor pose (it fixes the gauge); frame i starts from T_i0 = T_i,in T_j,in^-1 T_j,trk
    // (world -> camera, j the previous fused frame), is registered in depth geometry and integrated at the result (T_i0 when the status is 2 or 3)
    const bool track = std::atoi(yaml(fusion_cfg, "track_frames", "0").c_str()) != 0;
    const std::string tracked_file = yaml(fusion_cfg, "output_tracked_poses");
    i3d_track_desc tdesc; i3d_track_desc_default(&tdesc);
    tdesc.use_context_camera = 0;
    for (int k = 0; k < 4; ++k) tdesc.intrinsics4[k] = di[k];
    for (int k = 0; k < 5; ++k) tdesc.distortion5[k] = 0.0;
    // opt-in "track_mode: sdf": the frames are registered on the volume's field itself (i3d_fusion_track_sdf, no ray cast); "icp" (default): i3d_fusion_track;
    // "sdf_rgbd": the same with the volume's fused colour (i3d_fusion_track_sdf_rgbd), the frame's luminance formed here at the depth camera's geometry
    const std::string track_mode = yaml(fusion_cfg, "track_mode", "icp");
    if (track && track_mode != "icp" && track_mode != "sdf" && track_mode != "sdf_rgbd") {
        std::fprintf(stderr, "track_mode must be \"icp\", \"sdf\" or \"sdf_rgbd\"\n"); return 1;
    }
    const bool track_sdf = track_mode == "sdf", track_sdf_rgbd = track_mode == "sdf_rgbd";
    i3d_track_sdf_desc sdesc; i3d_track_sdf_desc_default(&sdesc);
    for (int k = 0; k < 4; ++k) sdesc.intrinsics4[k] = di[k];
    i3d_track_sdf_rgbd_desc pdesc; i3d_track_sdf_rgbd_desc_default(&pdesc);
    pdesc.base = sdesc;
    const std::string photo_weight = yaml(fusion_cfg, "track_photo_weight");
    if (!photo_weight.empty()) pdesc.photo_weight = std::atof(photo_weight.c_str());
    std::vector<float> lum(track && track_sdf_rgbd ? (size_t)dwh[0] * dwh[1] : 0);
    double prev_in[16], prev_trk[16]; bool have_prev = false; int registered = 0, kept = 0;
    std::vector<float> depth((size_t)dwh[0] * dwh[1]), pose(16); std::vector<uint8_t> bgr((size_t)cwh[0] * cwh[1] * 3);
    // one registration of the frame in `depth` / `bgr` against the volume as it stands by the tracker of track_mode; the figures every tracker has go to st
    auto register_frame = [&](double* p6, i3d_track_stats& st) -> bool {
        if (track_sdf) {
            i3d_track_sdf_stats ss; std::memset(&ss, 0, sizeof(ss));
            if (i3d_fusion_track_sdf(vol, &sdesc, dwh[0], dwh[1], depth.data(), p6, &ss) != I3D_OK) {
                std::fprintf(stderr, "Frame tracking failed! %s\n", i3d_fusion_last_error(vol)); return false;
            }
            st.status = ss.status; st.iterations[0] = ss.iterations; st.inliers = ss.inliers; st.valid_pixels = ss.valid_pixels;
            st.rms_initial = ss.rms_initial; st.rms_final = ss.rms_final;
        } else if (track_sdf_rgbd) {
            i3d_track_sdf_rgbd_stats ps; std::memset(&ps, 0, sizeof(ps));
            luminance_at_depth_geometry(bgr.data(), cwh, ci, dwh, di, lum.data());
            if (i3d_fusion_track_sdf_rgbd(vol, &pdesc, dwh[0], dwh[1], depth.data(), lum.data(), p6, &ps) != I3D_OK) {
                std::fprintf(stderr, "Frame tracking failed! %s\n", i3d_fusion_last_error(vol)); return false;
            }
            st.status = ps.base.status; st.iterations[0] = ps.base.iterations; st.inliers = ps.base.inliers; st.valid_pixels = ps.base.valid_pixels;
            st.rms_initial = ps.base.rms_initial; st.rms_final = ps.base.rms_final;
            std::printf("   photometric: %lld samples, rms %.3g -> %.3g\n", (long long)ps.photo_samples, ps.photo_rms_initial, ps.photo_rms_final);
        } else if (i3d_fusion_track(vol, &tdesc, dwh[0], dwh[1], depth.data(), p6, &st) != I3D_OK) {
            std::fprintf(stderr, "Frame tracking failed! %s\n", i3d_fusion_last_error(vol)); return false;
        }
        return true;
    };
    // opt-in leave-one-out passes after the sequence: the fused frames and the ordinals the volume knows them by
    const int repose_passes = std::atoi(yaml(fusion_cfg, "repose_passes", "0").c_str());
    if (repose_passes < 0 || (repose_passes > 0 && !track)) { std::fprintf(stderr, "repose_passes needs track_frames: \"1\" and a count >= 0\n"); return 1; }
    std::vector<int> fused_frame; std::vector<uint64_t> fused_ordinal;
    std::printf("Fusion...\n");
    for (int i = 0; i < num_frames; ++i) {
        if (use_kf && !((size_t)i < is_kf.size() && is_kf[i])) continue;
        std::printf("   integrating frame %d... \n", i);
        if (i3d_sensor_depth(sensor, i, depth.data()) != I3D_OK || i3d_sensor_color(sensor, i, bgr.data()) != I3D_OK) continue;       // a frame that was not loaded: empty cv::Mat in the reference
        i3d_sensor_pose(sensor, i, pose.data());
        if (track) {
            double in_c2w[16], t_in[16];
            for (int e = 0; e < 16; ++e) in_c2w[e] = pose[e];
            rigid_inverse(in_c2w, t_in);
            if (have_prev) {
                double prev_in_inv[16], tmp[16], t0[16], c2w0[16];
                rigid_inverse(prev_in, prev_in_inv);
                mat_mul(t_in, prev_in_inv, tmp); mat_mul(tmp, prev_trk, t0);
                rigid_inverse(t0, c2w0);
                float c2w0f[16]; for (int e = 0; e < 16; ++e) c2w0f[e] = (float)c2w0[e];
                double guess[6], p6[6]; i3d_pose_mat_to_vec6(c2w0f, guess);
                for (int e = 0; e < 6; ++e) p6[e] = guess[e];
                i3d_track_stats st; std::memset(&st, 0, sizeof(st));
                if (!register_frame(p6, st)) return 1;
                std::printf("   tracking frame %d: status %d, %d iterations, %lld inliers of %lld pixels, rms %.3g -> %.3g m\n", i, st.status, st.iterations[0],
                            (long long)st.inliers, (long long)st.valid_pixels, st.rms_initial, st.rms_final);
                if (st.status == 0 || st.status == 1) ++registered; else { for (int e = 0; e < 6; ++e) p6[e] = guess[e]; ++kept; }
                i3d_sensor_set_pose_vec6(sensor, i, p6);                  // the trajectory, and the Mat4f that integrate takes
                i3d_sensor_pose(sensor, i, pose.data());
                mat_from_vec6(p6, prev_trk);
            } else {
                for (int e = 0; e < 16; ++e) prev_trk[e] = t_in[e];
            }
            for (int e = 0; e < 16; ++e) prev_in[e] = t_in[e];
            have_prev = true;
        }
        uint64_t ordinal = 0; i3d_fusion_info(vol, &ordinal, nullptr, nullptr, nullptr);      // the ordinal of the integrate that follows
        if (i3d_fusion_integrate(vol, dwh[0], dwh[1], di, cwh[0], cwh[1], ci, depth.data(), bgr.data(), pose.data(), erode) != I3D_OK) {
            std::fprintf(stderr, "SDF fusion failed! %s\n", i3d_fusion_last_error(vol)); return 1;
        }
        fused_frame.push_back(i); fused_ordinal.push_back(ordinal);
        if (prune_every > 0 && fused_frame.size() % (size_t)prune_every == 0) {
            int64_t pc[5] = {0, 0, 0, 0, 0};
            if (i3d_fusion_prune(vol, prune_min_weight, prune_max_sdf, 0, nullptr, 1, pc) != I3D_OK) {
                std::fprintf(stderr, "Prune failed! %s\n", i3d_fusion_last_error(vol)); return 1;
            }
            std::printf("   prune after frame %d: %lld of %lld voxels removed\n", i, (long long)pc[1], (long long)pc[0]);
        }
        if (checkpoint_every > 0 && fused_frame.size() % (size_t)checkpoint_every == 0) {
            uint64_t kept_voxels = 0;
            if (i3d_fusion_snapshot(vol, &kept_voxels) != I3D_OK || i3d_fusion_save(vol, checkpoint_file.c_str()) != I3D_OK) {
                std::fprintf(stderr, "Checkpoint failed! %s\n", i3d_fusion_last_error(vol)); return 1;
            }
            std::printf("   checkpoint after frame %d: %llu voxels to %s\n", i, (unsigned long long)kept_voxels, checkpoint_file.c_str());
        }
    }
    for (int pass = 1; pass <= repose_passes; ++pass) {
        std::printf("repose pass %d ...\n", pass);
        int moved = 0;
        for (size_t k = 1; k < fused_frame.size(); ++k) {                // the first fused frame keeps its pose: it fixes the gauge
            const int i = fused_frame[k];
            if (i3d_sensor_depth(sensor, i, depth.data()) != I3D_OK || i3d_sensor_color(sensor, i, bgr.data()) != I3D_OK) continue;
            i3d_sensor_pose(sensor, i, pose.data());                     // the pose the frame is in the volume at
            if (i3d_fusion_deintegrate(vol, fused_ordinal[k], dwh[0], dwh[1], di, cwh[0], cwh[1], ci, depth.data(), bgr.data(), pose.data(), erode) != I3D_OK) {
                std::fprintf(stderr, "SDF fusion failed! %s\n", i3d_fusion_last_error(vol)); return 1;
            }
            double guess[6], p6[6]; i3d_pose_mat_to_vec6(pose.data(), guess);
            for (int e = 0; e < 6; ++e) p6[e] = guess[e];
            i3d_track_stats st; std::memset(&st, 0, sizeof(st));
            if (!register_frame(p6, st)) return 1;
            std::printf("   reposing frame %d: status %d, %d iterations, %lld inliers of %lld pixels, rms %.3g -> %.3g m\n", i, st.status, st.iterations[0],
                        (long long)st.inliers, (long long)st.valid_pixels, st.rms_initial, st.rms_final);
            if (st.status == 0 || st.status == 1) { i3d_sensor_set_pose_vec6(sensor, i, p6); i3d_sensor_pose(sensor, i, pose.data()); ++moved; }
            i3d_fusion_info(vol, &fused_ordinal[k], nullptr, nullptr, nullptr);
            if (i3d_fusion_integrate(vol, dwh[0], dwh[1], di, cwh[0], cwh[1], ci, depth.data(), bgr.data(), pose.data(), erode) != I3D_OK) {
                std::fprintf(stderr, "SDF fusion failed! %s\n", i3d_fusion_last_error(vol)); return 1;
            }
        }
        std::printf("   %d of %zu frames moved\n", moved, fused_frame.size() > 0 ? fused_frame.size() - 1 : (size_t)0);
    }
    if (track) std::printf("Tracking: %d frames registered, %d integrated at their predicted pose (status 2 / 3)\n", registered, kept);
    if (!tracked_file.empty()) {
        std::printf("Saving camera poses to file %s ...\n", tracked_file.c_str());
        if (i3d_sensor_save_poses(sensor, tracked_file.c_str()) != I3D_OK) std::fprintf(stderr, "Could not save tracked poses...\n");
    }
    if (components_min_voxels > 0) {
        int64_t cc[5] = {0, 0, 0, 0, 0};
        if (i3d_fusion_prune_components(vol, 0.0f, 0.0f, (int64_t)components_min_voxels, 0, 1, cc) != I3D_OK) {
            std::fprintf(stderr, "Component prune failed! %s\n", i3d_fusion_last_error(vol)); return 1;
        }
        std::printf("components: %lld of %lld with fewer than %lld voxels removed, %lld of %lld voxels\n", (long long)cc[4], (long long)cc[3],
                    components_min_voxels, (long long)cc[1], (long long)cc[0]);
    }
    // opt-in "output_mesh_live": an indexed mesh of the volume as it stands, before correctSDF (i3d_fusion_extract_mesh)
    const std::string live_mesh_file = yaml(fusion_cfg, "output_mesh_live");
    if (!live_mesh_file.empty()) {
        std::printf("Saving mesh of the live volume to file %s ...\n", live_mesh_file.c_str());
        i3d_fusion_mesh_desc mdesc; i3d_fusion_mesh_desc_default(&mdesc);
        if (i3d_fusion_export_mesh_ply(vol, &mdesc, live_mesh_file.c_str()) != I3D_OK) std::fprintf(stderr, "Mesh of the live volume could not be saved! %s\n", i3d_fusion_last_error(vol));
    }
    std::printf("correct SDF ...\nclear invalid voxels ...\n");
    uint64_t count = 0;
    if (i3d_fusion_finish(vol, correct_iterations, &count) != I3D_OK) { std::fprintf(stderr, "SDF fusion failed! %s\n", i3d_fusion_last_error(vol)); return 1; }
    std::printf("Saving SDF (%llu voxels) ...\n", (unsigned long long)count);
    const std::string sdf_file = yaml(fusion_cfg, "output_sdf");
    if (!sdf_file.empty() && i3d_fusion_save(vol, sdf_file.c_str()) != I3D_OK) std::fprintf(stderr, "Could not save SDF volume to file ...\n");

    std::printf("Saving mesh ...\n");
    const std::string mesh_file = yaml(fusion_cfg, "output_mesh");
    if (!mesh_file.empty() && count > 0) {
        std::vector<int32_t> keys(3 * count); std::vector<float> sdf(count), weight(count); std::vector<uint8_t> color(3 * count);
        i3d_fusion_get(vol, keys.data(), sdf.data(), weight.data(), color.data());
        // MarchingCubes<Voxel>::extractSurface(*grid) walks the FUSION grid itself (app_fusion.cpp:186-193): its visit order is the record order of the
        // volume — not the order a load + convert of the saved file would give (what i3d_set_grid_from_tsdf_records restates for the refinement app)
        std::vector<double> sdf_d(sdf.begin(), sdf.end()), albedo(count, 0.0);
        i3d_grid_view gv; gv.num_voxels = (int64_t)count; gv.voxel_size = voxel_size; gv.truncation = voxel_size * 5.0f; gv.keys = keys.data();
        gv.sdf = sdf_d.data(); gv.sdf_refined = sdf_d.data(); gv.albedo = albedo.data(); gv.weight = weight.data(); gv.color = color.data();
        i3d_context* ctx = nullptr;
        if (i3d_create(device, &ctx) != I3D_OK || i3d_set_grid(ctx, &gv) != I3D_OK)
            std::fprintf(stderr, "Mesh could not be generated!\n");
        else if (i3d_export_mesh_ply(ctx, mesh_file.c_str(), 0, 0, 0) != I3D_OK) std::fprintf(stderr, "Mesh could not be saved!\n");
        if (ctx) i3d_destroy(ctx);
    }
    i3d_fusion_destroy(vol); i3d_sensor_close(sensor);
    return 0;
}
