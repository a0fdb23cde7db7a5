// radiance_orc.cpp -- TEST TOOLING: what vrt_trace_radiance (include/vrt_api.h) must return, computed by the oracle alone.  The oracle
// has no entry point for caller-supplied rays; its render body for ONE pixel is public (orc::Renderer::render_pixel), and so are the
// frame counter and the two colour buffers.  This translation unit includes the oracle's sources unchanged -- so the library it builds
// into (tests/emul/_radiance_orc.so, tests/radiance.py) carries every orc_* entry point -- and adds one function: for pixel (u, v)
// of a context set up through the ordinary orc_* calls with ReSTIR off, a static camera and render scale 1, sample s is render_pixel
// with current_frame = first_frame + s; the two colours it leaves are scrubbed by the temporal prepass's rule (scrub_needed) and
// added, and the samples are summed in order and divided by their number, in binary32.  The rays of a test are the camera rays of that
// context, (camera_pos, orc_unit_cast_dir(u, v)) with stream v * W + u: the query must reproduce what the reference's render body
// computes for them.
#include "../../oracle/orc_api.cpp"

extern "C" {

// uv: n pairs (u, v); out: n x 3 floats.  -1: the context is not in the state stated above, or a pixel lies outside the frame.
int orc_radiance_pixels(orc_ctx* c, int n, const int32_t* uv, int n_samples, uint32_t first_frame, float* out) {
    Renderer& r = c->r;
    if (r.use_restir || r.camera_is_moving != 0 || r.render_scale != 1.0f || n_samples < 1) return -1;
    const uint32_t keep = r.current_frame;
    for (int k = 0; k < n; k++) {
        const int u = uv[2 * k], v = uv[2 * k + 1];
        if (u < 0 || v < 0 || u >= r.W || v >= r.H) { r.current_frame = keep; return -1; }
        const size_t pix = (size_t)v * r.W + u;
        V3 sum = v3(0.0f);
        for (int s = 0; s < n_samples; s++) {
            r.current_frame = first_frame + (uint32_t)s;
            r.render_pixel(u, v, nullptr);
            V3 d = r.color_buffer[pix], sp = r.color_buffer_specular[pix];
            if (Renderer::scrub_needed(d)) d = v3(0.0f);
            if (Renderer::scrub_needed(sp)) sp = v3(0.0f);
            const V3 value = d + sp;
            sum.x += value.x; sum.y += value.y; sum.z += value.z;
        }
        out[3 * k] = sum.x / (float)n_samples; out[3 * k + 1] = sum.y / (float)n_samples; out[3 * k + 2] = sum.z / (float)n_samples;
    }
    r.current_frame = keep;
    return 0;
}

// Census only: the voxel walks (closest-hit and shadow rays) sample `frame` of each pixel takes.  A path still alive at segment d takes
// at least one walk more with max_depth = d + 1 than with max_depth = d, and a path that ended earlier takes the same number.
int orc_radiance_walks(orc_ctx* c, int n, const int32_t* uv, uint32_t frame, uint32_t* out) {
    Renderer& r = c->r;
    const uint32_t keep = r.current_frame;
    r.current_frame = frame;
    for (int k = 0; k < n; k++) {
        Stats st;
        r.render_pixel(uv[2 * k], uv[2 * k + 1], &st);
        out[k] = (uint32_t)st.rays;
    }
    r.current_frame = keep;
    return 0;
}

}  // extern "C"
