// preint_cpu.cpp -- IMU pre-integration on ONE host core: the single-threaded yardstick of tools/preint_timing.py, and what
// tests/test_imu_preint_reference.py holds to the numpy reference without a device.  The arithmetic is csrc/imu_preint_math.h, the
// very functions the kernels of csrc/imu_preintegrate.hip run one lane each; here a plain loop runs them one after the other.
//   g++ -O3 -ffp-contract=off -fPIC -shared -std=c++17 -I include -o libpreint_cpu.so tools/preint_cpu.cpp
#include "../orb_slam3-1_amd/csrc/imu_preint_math.h"

extern "C" {

void preint_cpu_preintegrate(ImuPreintState* states, int n_states, const ImuPreintJob* jobs, int n_jobs, const ImuMeasurement* meas, int n_meas, int32_t* status)
{
    for (int j = 0; j < n_jobs; j++) preint::preintegrate_job(states, n_states, jobs, n_jobs, meas, n_meas, status, j, false);
}

void preint_cpu_frame_measurements(const OrbeImuSample* samples, const int32_t* n_imu, const int64_t* t_prev_ns, const int64_t* t_cur_ns, int batch, int imu_cap,
                                   ImuMeasurement* meas_out, int32_t* count_out)
{
    for (int b = 0; b < batch; b++)
        for (int i = 0; i < (imu_cap > 1 ? imu_cap : 1); i++) preint::frame_measurement(samples, n_imu, t_prev_ns, t_cur_ns, imu_cap, meas_out, count_out, b, i);
}

void preint_cpu_links(const ImuPreintState* states, int n_states, const ImuLinkSpec* specs, int n_links, LibaLink* links, int32_t* status)
{
    for (int l = 0; l < n_links; l++) preint::build_link(states, n_states, specs, links, status, l);
}

void preint_cpu_predict(const ImuPreintState* states, int n_states, const ImuPredictJob* jobs, int n_jobs, ImuPredictOut* out, int32_t* status)
{
    for (int j = 0; j < n_jobs; j++) preint::predict_job(states, n_states, jobs, out, status, j);
}

}  // extern "C"
