// AppIntrinsic3D on the MI355X library: the caller of the drop-in boundary (apps/src/app_intrinsic3d.cpp:72-210 of the reference),
// written against include/intrinsic3d_hip.h only.
//
//   app_intrinsic3d -s <path>/sensor.yml -i <path>/intrinsic3d.yml [--device N]
//
// sensor.yml / intrinsic3d.yml are the reference's files (data/*.yml).  As in the reference the working directory becomes the directory of
// sensor.yml, ./intrinsic3d is created, and after every (grid level, rgbd level) the meshes, poses and intrinsics are written with the
// `_g{L}_p{P}` postfix.  Opt-in, not in the reference: `output_tracked_poses_prefix` also registers every non-keyframe against the model of that level
// (i3d_track_frame) and writes all frames' poses, keyframes refined, in Sensor::savePoses layout; with `tracked_poses_photo_weight: "<w_p>"` > 0 next to it the
// registration also uses the frame's colour against the model's predicted intensity (i3d_track_frame_rgbd, photo weight w_p).  Mesh colour modes: every `output_mesh_*` switch of intrinsic3d.yml except the two subvolume views (random colours in the reference).
#include "../include/intrinsic3d_hip.h"
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
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
std::string absolute(const std::string& p) { char buf[PATH_MAX]; return realpath(p.c_str(), buf) ? std::string(buf) : p; }

struct App {
    i3d_context* ctx = nullptr;
    i3d_sensor* sensor = nullptr;
    std::string cfg_file;
    std::vector<int32_t> frame_ids;
    int color_w = 0, color_h = 0, depth_w = 0, depth_h = 0, device = 0, num_frames = 0;
    float color_intr[4] = {0, 0, 0, 0}, depth_intr[4] = {0, 0, 0, 0};
    std::vector<float> input_c2w;                  // [num_frames][16] the sensor's poses before refinement
};

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
void mat_mul(const double* x, const double* y, double* o) {
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) { double s = 0.0; for (int k = 0; k < 4; ++k) s += x[4 * a + k] * y[4 * k + b]; o[4 * a + b] = s; }
}

// every non-keyframe registered against the model of this level; the initial guess is the input pose corrected by the nearest keyframe's refinement,
// T_i0 = T_i,in T_k,in^-1 T_k,ref (world -> camera).  The sensor's poses are restored afterwards: only the file carries the tracked poses.
void save_tracked_poses(App& a, const std::string& file, const std::vector<double>& poses, double photo_weight) {
    const int n = a.num_frames, nk = (int)a.frame_ids.size();
    std::vector<int> kf_of(n, -1);
    for (int k = 0; k < nk; ++k) if (a.frame_ids[k] >= 0 && a.frame_ids[k] < n) kf_of[a.frame_ids[k]] = k;
    std::vector<float> saved(16 * (size_t)n);
    for (int i = 0; i < n; ++i) i3d_sensor_pose(a.sensor, i, &saved[16 * (size_t)i]);
    i3d_track_desc desc; i3d_track_desc_default(&desc);
    i3d_track_rgbd_desc rgbd; i3d_track_rgbd_desc_default(&rgbd);        // its base: the defaults above, the refined sdf, the context's refined camera
    rgbd.photo_weight = photo_weight;
    const bool photo = photo_weight > 0.0;
    std::vector<float> raw((size_t)a.depth_w * a.depth_h), depth((size_t)a.color_w * a.color_h), lum(photo ? depth.size() : 0);
    std::vector<uint8_t> bgr(photo ? 3 * depth.size() : 0);
    // the frame's luminance as the keyframes' level 0 has it (the loader's conversion: 1 / 255, then 0.114 B + 0.587 G + 0.299 R in float)
    auto luminance = [&](int i) {
        if (i3d_sensor_color(a.sensor, i, bgr.data()) != I3D_OK) return false;
        const float sc = (float)(1.0 / 255.0);
        for (size_t p = 0; p < lum.size(); ++p) {
            const float b = (float)bgr[3 * p] * sc, g = (float)bgr[3 * p + 1] * sc, r = (float)bgr[3 * p + 2] * sc;
            lum[p] = (b * 0.114f + g * 0.587f) + r * 0.299f;
        }
        return true;
    };
    int kept = 0, tracked = 0;
    for (int i = 0; i < n && nk > 0; ++i) {
        if (kf_of[i] >= 0) continue;
        int k = 0;
        for (int j = 1; j < nk; ++j) if (std::abs(a.frame_ids[j] - i) < std::abs(a.frame_ids[k] - i)) k = j;
        double in_c2w_i[16], in_c2w_k[16], t_in_i[16], t_ref_k[16], tmp[16], t0[16], c2w0[16];
        for (int e = 0; e < 16; ++e) { in_c2w_i[e] = a.input_c2w[16 * (size_t)i + e]; in_c2w_k[e] = a.input_c2w[16 * (size_t)a.frame_ids[k] + e]; }
        rigid_inverse(in_c2w_i, t_in_i);
        mat_from_vec6(&poses[6 * (size_t)k], t_ref_k);
        mat_mul(t_in_i, in_c2w_k, tmp); mat_mul(tmp, t_ref_k, t0);
        rigid_inverse(t0, c2w0);
        float c2w0f[16]; for (int e = 0; e < 16; ++e) c2w0f[e] = (float)c2w0[e];
        double guess[6]; i3d_pose_mat_to_vec6(c2w0f, guess);
        double pose[6]; for (int e = 0; e < 6; ++e) pose[e] = guess[e];
        i3d_track_stats st; std::memset(&st, 0, sizeof(st));
        i3d_track_rgbd_stats rst; std::memset(&rst, 0, sizeof(rst));
        bool ok = i3d_sensor_depth(a.sensor, i, raw.data()) == I3D_OK &&
                  i3d_resize_depth(a.device, a.depth_w, a.depth_h, raw.data(), a.depth_intr, a.color_w, a.color_h, a.color_intr, depth.data()) == I3D_OK;
        if (ok && photo) {
            ok = luminance(i) && i3d_track_frame_rgbd(a.ctx, &rgbd, a.color_w, a.color_h, depth.data(), lum.data(), pose, &rst) == I3D_OK;
            st = rst.base;
        } else if (ok) {
            ok = i3d_track_frame(a.ctx, &desc, a.color_w, a.color_h, depth.data(), pose, &st) == I3D_OK;
        }
        ok = ok && (st.status == 0 || st.status == 1);
        std::printf("   frame %d: status %d, %d iterations, %lld inliers of %lld pixels, rms %.3g -> %.3g m\n", i, st.status, st.iterations[0],
                    (long long)st.inliers, (long long)st.valid_pixels, st.rms_initial, st.rms_final);
        if (photo) std::printf("      %lld photometric samples, luminance rms %.3g -> %.3g\n", (long long)rst.photo_samples, rst.photo_rms_initial, rst.photo_rms_final);
        if (!ok) { for (int e = 0; e < 6; ++e) pose[e] = guess[e]; ++kept; } else ++tracked;
        i3d_sensor_set_pose_vec6(a.sensor, i, pose);
    }
    std::printf("Saving tracked camera poses to file %s (%d frames registered, %d kept their initial guess)\n", file.c_str(), tracked, kept);
    if (i3d_sensor_save_poses(a.sensor, file.c_str()) != I3D_OK) std::fprintf(stderr, "Could not save tracked poses...\n");
    for (int i = 0; i < n; ++i) i3d_sensor_set_pose(a.sensor, i, &saved[16 * (size_t)i]);
}

// AppIntrinsic3D::onSDFRefined (app_intrinsic3d.cpp:159-210) + the write-back of Intrinsic3D::finishRgbdLevel (intrinsic3d.cpp:362-372)
void on_refined(void* user, int32_t grid_level, int32_t, int32_t pyramid_level, int32_t) {
    App& a = *static_cast<App*>(user);
    const std::string post = "_g" + std::to_string(grid_level) + "_p" + std::to_string(pyramid_level);
    const std::string mesh_prefix = yaml(a.cfg_file, "output_mesh_prefix");
    if (!mesh_prefix.empty()) {
        const int largest = std::atoi(yaml(a.cfg_file, "output_mesh_largest_comp_only", "0").c_str());
        // SDFVisualization::getOutputModes(settings, true) (sdf/visualization.cpp:71-89): the voxel colours, then every enabled mode in this order
        static const struct { const char* key; const char* name; int mode; } MODES[] = {
            {nullptr, "", I3D_COLOR_VOXEL}, {"output_mesh_normals", "normals", I3D_COLOR_NORMALS}, {"output_mesh_laplacian", "lap", I3D_COLOR_LAPLACIAN},
            {"output_mesh_intensity", "lum", I3D_COLOR_INTENSITY}, {"output_mesh_intensity_grad", "lum_grad", I3D_COLOR_INTENSITY_GRAD}, {"output_mesh_albedo", "albedo", I3D_COLOR_ALBEDO},
            {"output_mesh_shading_sv", "shading_sv", I3D_COLOR_SHADING}, {"output_mesh_shading_sv_const", "shading_sv_const", I3D_COLOR_SHADING_CONST_ALBEDO},
            {"output_mesh_chromacity", "chroma", I3D_COLOR_CHROMACITY}};
        for (const auto& m : MODES) {
            if (m.key && !std::atoi(yaml(a.cfg_file, m.key, "0").c_str())) continue;
            std::printf("SDF visualization and export: %s\n", m.name);
            const std::string file = mesh_prefix + post + (m.name[0] ? "_" + std::string(m.name) : std::string()) + ".ply";
            if (i3d_export_mesh_ply(a.ctx, file.c_str(), 1, m.mode, largest) != I3D_OK) std::fprintf(stderr, "Could not save mesh: %s\n", i3d_last_error(a.ctx));
        }
        for (const char* key : {"output_mesh_subvolumes", "output_mesh_subvolumes_interpolated"})           // painted with rand() colours in the reference: nothing to reproduce
            if (std::atoi(yaml(a.cfg_file, key, "0").c_str())) std::fprintf(stderr, "%s: this view shows random subvolume colours in the reference and is not produced here\n", key);
    }
    double intr[4], dist[5]; std::vector<double> poses(6 * a.frame_ids.size());
    if (i3d_get_camera(a.ctx, intr, dist, poses.data()) != I3D_OK) { std::fprintf(stderr, "Could not read the camera: %s\n", i3d_last_error(a.ctx)); return; }
    for (size_t k = 0; k < a.frame_ids.size(); ++k) i3d_sensor_set_pose_vec6(a.sensor, a.frame_ids[k], &poses[6 * k]);
    const std::string poses_prefix = yaml(a.cfg_file, "output_poses_prefix");
    if (!poses_prefix.empty()) {
        const std::string file = poses_prefix + post + ".txt";
        std::printf("Saving camera poses to file %s\n", file.c_str());
        if (i3d_sensor_save_poses(a.sensor, file.c_str()) != I3D_OK) std::fprintf(stderr, "Could not save poses...\n");
    }
    const std::string intr_prefix = yaml(a.cfg_file, "output_intrinsics_prefix");
    if (!intr_prefix.empty()) {
        const std::string file = intr_prefix + post + ".txt";
        std::printf("Saving camera intrinsics to file %s\n", file.c_str());
        if (i3d_write_intrinsics(file.c_str(), a.color_w, a.color_h, intr, dist) != I3D_OK) std::fprintf(stderr, "Could not save color camera intrinsics!\n");
    }
    const std::string tracked_prefix = yaml(a.cfg_file, "output_tracked_poses_prefix");
    if (!tracked_prefix.empty()) save_tracked_poses(a, tracked_prefix + post + ".txt", poses, std::atof(yaml(a.cfg_file, "tracked_poses_photo_weight", "0").c_str()));
    std::fflush(stdout);
}

}  // namespace

int main(int argc, char* argv[]) {
    std::string sensor_cfg, i3d_cfg; int device = 0;
    for (int i = 1; i < argc; ++i) {                            // cv::CommandLineParser accepts -s=<v> / --sensor=<v>; `-s <v>` is accepted as well
        std::string arg = argv[i], val; const size_t eq = arg.find('=');
        if (eq != std::string::npos) { val = arg.substr(eq + 1); arg = arg.substr(0, eq); } else if (i + 1 < argc) val = argv[++i];
        if (arg == "-s" || arg == "--sensor") sensor_cfg = val;
        else if (arg == "-i" || arg == "--intrinsic3d") i3d_cfg = val;
        else if (arg == "--device") device = std::atoi(val.c_str());
        else { std::fprintf(stderr, "usage: %s -s <sensor.yml> -i <intrinsic3d.yml> [--device N]\n", argv[0]); return 2; }
    }
    if (sensor_cfg.empty() || i3d_cfg.empty()) { std::fprintf(stderr, "usage: %s -s <sensor.yml> -i <intrinsic3d.yml> [--device N]\n", argv[0]); return 2; }
    sensor_cfg = absolute(sensor_cfg); i3d_cfg = absolute(i3d_cfg);
    const std::string dir = sensor_cfg.substr(0, sensor_cfg.find_last_of('/'));
    if (chdir(dir.c_str()) != 0) { std::fprintf(stderr, "cannot change the working directory to %s\n", dir.c_str()); return 1; }
    mkdir("./intrinsic3d", 0755);

    App app; app.cfg_file = i3d_cfg;
    int rc = i3d_sensor_open_yaml(sensor_cfg.c_str(), &app.sensor, nullptr, nullptr);                      // Sensor::create(sensor_cfg)
    int32_t num_frames = 0, num_loaded = 0, cwh[2] = {0, 0}, dwh[2] = {0, 0};
    if (rc == I3D_OK) i3d_sensor_info(app.sensor, &num_frames, &num_loaded, cwh, dwh, app.color_intr, app.depth_intr);
    if (rc != I3D_OK || num_loaded == 0) { std::fprintf(stderr, "RGB-D sensor could not be initialized!\n"); return 1; }
    app.color_w = cwh[0]; app.color_h = cwh[1]; app.depth_w = dwh[0]; app.depth_h = dwh[1]; app.device = device; app.num_frames = num_frames;
    app.input_c2w.resize(16 * (size_t)num_frames);
    for (int i = 0; i < num_frames; ++i) i3d_sensor_pose(app.sensor, i, &app.input_c2w[16 * (size_t)i]);
    std::printf("%d filenames loaded.\n", num_frames);

    i3d_refine_config rcfg; i3d_optimizer_config ocfg;
    std::memset(&rcfg, 0, sizeof(rcfg)); i3d_optimizer_config_default(&ocfg);
    rcfg.num_grid_levels = 3; rcfg.num_rgbd_levels = 3; rcfg.thin_shell_factor = 2.0; rcfg.thin_shell_factor_final = 1.0; rcfg.clear_distant_voxels = 1;   // Intrinsic3D::Config
    rcfg.occlusion_distance = 0.02f; rcfg.num_observations = 5; rcfg.subvolume_size_sh = 0.2f; rcfg.sh_lambda_reg = 10.0;                                   // (intrinsic3d.h:67-83)
    if (i3d_config_load_yaml(i3d_cfg.c_str(), &rcfg, &ocfg) != I3D_OK) { std::fprintf(stderr, "Could not load %s\n", i3d_cfg.c_str()); return 1; }

    std::printf("Loading Keyframes...\n");
    int32_t window = 0; uint64_t nkf_lines = 0;
    std::vector<uint8_t> is_kf;
    const std::string kf_file = yaml(i3d_cfg, "keyframes");
    if (i3d_keyframes_load(kf_file.c_str(), &window, 0, nullptr, nullptr, &nkf_lines) == I3D_OK) {
        is_kf.resize(nkf_lines);
        i3d_keyframes_load(kf_file.c_str(), &window, nkf_lines, nullptr, is_kf.data(), &nkf_lines);
    } else std::fprintf(stderr, "Could not load keyframes ...\n");
    size_t nkf = 0; for (uint8_t k : is_kf) nkf += k != 0;
    std::printf("%zu keyframes loaded.\n", nkf);

    std::printf("Loading SDF volume...\n");
    const std::string sdf_file = yaml(i3d_cfg, "input_sdf");
    float voxel_size = 0, truncation = 0, iws = 0, mlf = 0; uint64_t count = 0;
    if (i3d_tsdf_read_header(sdf_file.c_str(), &voxel_size, &truncation, &iws, &count, &mlf) != I3D_OK) { std::fprintf(stderr, "Could not load voxel grid!\n"); return 1; }
    std::vector<int32_t> keys(3 * count); std::vector<float> sdf(count), weight(count); std::vector<uint8_t> color(3 * count);
    if (i3d_tsdf_read_records(sdf_file.c_str(), count, keys.data(), sdf.data(), weight.data(), color.data()) != I3D_OK) { std::fprintf(stderr, "Could not load voxel grid!\n"); return 1; }
    std::printf("   %llu voxels, voxel size %g\n", (unsigned long long)count, (double)voxel_size);

    if (i3d_create(device, &app.ctx) != I3D_OK) { std::fprintf(stderr, "no HIP device %d\n", device); return 1; }
    auto fail = [&](const char* what) { std::fprintf(stderr, "%s: %s\n", what, i3d_last_error(app.ctx)); i3d_destroy(app.ctx); i3d_sensor_close(app.sensor); return 1; };
    if (i3d_set_grid_from_tsdf_records(app.ctx, voxel_size, count, keys.data(), sdf.data(), weight.data(), color.data()) != I3D_OK) return fail("Intrinsic3D failed (grid)");
    std::printf("   convert and store input frames ...\n");
    app.frame_ids.resize(nkf ? nkf : 1); int32_t nk = 0;
    if (i3d_init_frames_from_sensor(app.ctx, device, app.sensor, is_kf.size(), is_kf.data(), rcfg.num_rgbd_levels, (int32_t)app.frame_ids.size(), app.frame_ids.data(), &nk) != I3D_OK)
        return fail("Intrinsic3D failed (frames)");
    app.frame_ids.resize(nk);
    if (i3d_refine(app.ctx, &rcfg, &ocfg, on_refined, &app) != I3D_OK) return fail("Intrinsic3D failed!");
    i3d_destroy(app.ctx); i3d_sensor_close(app.sensor);
    return 0;
}
