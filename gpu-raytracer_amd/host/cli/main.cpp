// Headless `pathtracer` executable: the reference's command line (Src/Args.cpp:51-184) and the
// part of its main loop that matters without a window (Src/Main.cpp:75-150): load the scene,
// run update() / render() until sample_index reaches -N, write the frame (-o file.ppm | file.exr)
// and exit. Window, GUI and the interactive camera are out of scope.
//
// Options without a counterpart in the reference: --device <ordinal>, --devices <a,b,...> (one frame split over several
// GPUs: row tiles dealt round-robin, one RCCL all-gather per render(), host/FrameSplit.h), --bvh-cache <bool>
// (the reference always uses its .bvh caches; here they are opt-in), --merge-static <0..3> (the flattened static geometry of
// DESIGN.md 4.6; 0 = the reference's one-tree-per-mesh layout), --alpha-masks (cut-outs from the albedo textures' alpha), --batch <n> samples per
// submission (default 4; 1 = one render() per sample exactly like the reference loop).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../AO.h"
#include "../FrameSplit.h"
#include "../Pathtracer.h"
#include "../capi.h"
#include "../Exporters.h"

namespace {

struct Option {
	const char * short_name; // may be null
	const char * long_name;
	const char * help;
	int          argument_count;
	std::function<void(const char * value)> apply;
};

struct CommandLine {
	int  device = 0;
	std::vector<int> devices;   // --devices: more than one entry = tile split (FrameSplit)
	int  batch  = 4;
	bool help   = false;
	bool print_config = false;
	std::string noise_map;      // --noise-map
	std::string sample_map;     // --sample-map
	std::string denoise_noisy;  // --denoise-noisy
	bool denoise_option = false;   // an option that needs --denoise was given
	std::string firefly_map;         // --firefly-map
	std::string firefly_unfiltered;  // --firefly-unfiltered
	bool firefly_option = false;     // an option that needs --firefly-filter was given
	bool firefly_auto_option = false;   // an option that needs --firefly-auto-start was given
	bool noise_robust_option = false;   // an option that needs --noise-robust was given
};

[[noreturn]] void die(const std::string & message) {
	fprintf(stderr, "%s\n", message.c_str());
	exit(1);
}

int parse_int(const char * text, const char * what) {
	char * end = nullptr;
	long value = strtol(text, &end, 10);
	if (end == text || *end != '\0') die(std::string("invalid integer '") + text + "' for " + what);
	return int(value);
}

float parse_float(const char * text, const char * what) {
	char * end = nullptr;
	float value = strtof(text, &end);
	if (end == text || *end != '\0') die(std::string("invalid number '") + text + "' for " + what);
	return value;
}

bool parse_bool(const char * text) { // Args.cpp:19-37: anything unrecognised counts as true, with a message
	for (const char * t : { "true", "True", "TRUE", "1" })   if (strcmp(text, t) == 0) return true;
	for (const char * f : { "false", "False", "FALSE", "0" }) if (strcmp(text, f) == 0) return false;
	printf("Invalid boolean argument '%s'!\n", text);
	return true;
}

std::vector<Option> make_options(CommandLine & cl) {
	std::vector<Option> o;
	o.push_back({ "I", "integrator", "Choose the integrator type. Supported options: pathtracer, ao", 1, [](const char * v) {
		if      (strcmp(v, "pathtracer") == 0) cpu_config.integrator = IntegratorType::PATHTRACER;
		else if (strcmp(v, "ao") == 0)         cpu_config.integrator = IntegratorType::AO;
		else die(std::string("'") + v + "' is not a recognized integrator type! Supported options: pathtracer, ao");
	} });
	o.push_back({ "W", "width",   "Sets the width of the image",  1, [](const char * v) { cpu_config.initial_width  = parse_int(v, "--width"); } });
	o.push_back({ "H", "height",  "Sets the height of the image", 1, [](const char * v) { cpu_config.initial_height = parse_int(v, "--height"); } });
	o.push_back({ "b", "bounce",  "Sets the number of pathtracing bounces", 1, [](const char * v) {
		int b = parse_int(v, "--bounce");
		gpu_config.num_bounces = b < 0 ? 0 : (b > RT_MAX_BOUNCES - 1 ? RT_MAX_BOUNCES - 1 : b);
	} });
	o.push_back({ "N", "samples", "Sets a target number of samples to use", 1, [](const char * v) { cpu_config.output_sample_index = parse_int(v, "--samples"); } });
	o.push_back({ "o", "output",  "Sets path to output file. Supported formats: ppm, exr", 1, [](const char * v) { cpu_config.output_filename = v; } });
	o.push_back({ "s", "scene",   "Sets path to scene file. Supported formats: Mitsuba XML, OBJ, and PLY", 1, [](const char * v) { cpu_config.scene_filenames.push_back(v); } });
	o.push_back({ "S", "sky",     "Sets path to sky file. Supported formats: HDR", 1, [](const char * v) { cpu_config.sky_filename = v; } });
	// the reference gives --bvh the short name -b as well; --bounce is listed first and wins it
	o.push_back({ nullptr, "bvh", "Sets type of BLAS BVH used. Supported options: sah, sbvh, bvh4, bvh8", 1, [](const char * v) {
		if      (strcmp(v, "sah")  == 0) cpu_config.bvh_type = BVHType::BVH;
		else if (strcmp(v, "sbvh") == 0) cpu_config.bvh_type = BVHType::SBVH;
		else if (strcmp(v, "bvh4") == 0) cpu_config.bvh_type = BVHType::BVH4;
		else if (strcmp(v, "bvh8") == 0) cpu_config.bvh_type = BVHType::BVH8;
		else die(std::string("'") + v + "' is not a recognized BVH type! Supported options: sah, sbvh, bvh4, bvh8");
	} });
	o.push_back({ nullptr, "nee", "Enables or disables Next Event Estimation",        1, [](const char * v) { gpu_config.enable_next_event_estimation        = parse_bool(v); } });
	o.push_back({ nullptr, "mis", "Enables or disables Multiple Importance Sampling", 1, [](const char * v) { gpu_config.enable_multiple_importance_sampling = parse_bool(v); } });
	o.push_back({ nullptr, "sky-sampling", "Importance-samples the sky in NEE: 0 = off (default), (0, 1] = the sky's share of the light samples", 1, [](const char * v) {
		float p = parse_float(v, "--sky-sampling");
		if (!(p == 0.0f || (p > 0.0f && p <= 1.0f))) die("--sky-sampling must be 0 (off) or in (0, 1]");
		cpu_config.sky_sampling = p;
	} });
	o.push_back({ nullptr, "light-tree", "NEE picks a triangle emitter by a light tree from the shading point instead of by power alone (DESIGN.md 7.11): less noise with many lights", 0, [](const char *) { cpu_config.light_tree = 1; } });
	o.push_back({ nullptr, "fog", "A homogeneous fog volume inside the box <minx,miny,minz,maxx,maxy,maxz> (or off): scattering with light sampling at every scatter event", 1, [](const char * v) {
		if (grt_config_set_string("fog", v) != 0) die(std::string("--fog: ") + grt_last_error());
	} });
	o.push_back({ nullptr, "fog-sigma-a", "Absorption coefficient of the fog per unit length: one number or r,g,b (default 0)", 1, [](const char * v) {
		if (grt_config_set_string("fog_sigma_a", v) != 0) die(std::string("--fog-sigma-a: ") + grt_last_error());
	} });
	o.push_back({ nullptr, "fog-sigma-s", "Scattering coefficient of the fog per unit length: one number or r,g,b (default 0.1)", 1, [](const char * v) {
		if (grt_config_set_string("fog_sigma_s", v) != 0) die(std::string("--fog-sigma-s: ") + grt_last_error());
	} });
	o.push_back({ nullptr, "fog-g", "Henyey-Greenstein asymmetry of the fog in (-1, 1): 0 isotropic (default), towards 1 forward scattering", 1, [](const char * v) {
		float g = parse_float(v, "--fog-g");
		if (!(g > -1.0f && g < 1.0f)) die("--fog-g must lie in (-1, 1)");
		cpu_config.fog_g = g;
	} });
	o.push_back({ nullptr, "fog-density", "A density grid laid over the fog volume's box: a Mitsuba gridvolume file <file.vol> (float32, one channel) whose values scale the fog's sigmas voxel by voxel (or off)", 1, [](const char * v) {
		if (grt_config_set_string("fog_density", v) != 0) die(std::string("--fog-density: ") + grt_last_error());
	} });
	o.push_back({ nullptr, "fog-volumes", "1: a scene file's shape with a null BSDF and an interior homogeneous medium becomes the fog volume over its bounding box; 0 (default): loaded as before", 1, [](const char * v) {
		cpu_config.fog_volumes = parse_bool(v) ? 1 : 0;
	} });
	o.push_back({ nullptr, "delta-lights", "Point emitters of a scene file load as true point lights (intensity in W/sr) instead of tiny emissive spheres", 0, [](const char *) { cpu_config.delta_lights = 1; } });
	o.push_back({ nullptr, "delta-light-share", "Share of the light samples that goes to point, spot and directional emitters beside area emitters: 0 = by power (default), (0, 1]", 1, [](const char * v) {
		float p = parse_float(v, "--delta-light-share");
		if (!(p == 0.0f || (p > 0.0f && p <= 1.0f))) die("--delta-light-share must be 0 (by power) or in (0, 1]");
		cpu_config.delta_light_share = p;
	} });
	o.push_back({ nullptr, "noise-target", "Renders until the noise figure (DESIGN.md 7.5) is at or below <e>; -N becomes the cap on the sample count. The figure is asked for at burst boundaries only: the call drains the wavefront", 1, [](const char * v) {
		float e = parse_float(v, "--noise-target");
		if (!(e > 0.0f && e < 1e30f)) die("--noise-target must be finite and positive");
		cpu_config.noise_target = e;
	} });
	o.push_back({ nullptr, "noise-min-samples", "With --noise-target: never stop below this many samples (default 16)", 1, [](const char * v) {
		int n = parse_int(v, "--noise-min-samples");
		if (n < 2) die("--noise-min-samples must be at least 2");
		cpu_config.noise_min_samples = n;
	} });
	o.push_back({ nullptr, "noise-map", "Writes the per-pixel relative standard error as a one-channel EXR (pixels that take no part are 0)", 1, [&cl](const char * v) { cl.noise_map = v; } });
	o.push_back({ nullptr, "adaptive", "With --noise-target: after --noise-min-samples uniform samples, renders only the 16 x 16 cells whose noise is still above the target (DESIGN.md 7.6)", 0, [](const char *) { cpu_config.adaptive_sampling = 1; } });
	o.push_back({ nullptr, "adaptive-dilate", "With --adaptive: 1 (default) keeps the neighbours of a noisy cell active too, 0 does not", 1, [](const char * v) {
		int d = parse_int(v, "--adaptive-dilate");
		if (d != 0 && d != 1) die("--adaptive-dilate must be 0 or 1");
		cpu_config.adaptive_dilate = d;
	} });
	o.push_back({ nullptr, "denoise", "Filters the finished still by its measured variance (DESIGN.md 7.9): -o receives the denoised image. Keeps the noise estimate and the albedo, normal and position AOVs", 0, [](const char *) { cpu_config.denoise = 1; } });
	o.push_back({ nullptr, "denoise-iterations", "With --denoise: a-trous passes of step 1, 2, 4, ... (0..6, default 5)", 1, [&cl](const char * v) {
		int n = parse_int(v, "--denoise-iterations");
		if (n < 0 || n > 6) die("--denoise-iterations must be between 0 and 6");
		cpu_config.denoise_iterations = n; cl.denoise_option = true;
	} });
	o.push_back({ nullptr, "denoise-noisy", "With --denoise: also writes the unfiltered image to <file> (ppm, exr)", 1, [&cl](const char * v) { cl.denoise_noisy = v; cl.denoise_option = true; } });
	o.push_back({ nullptr, "firefly-filter", "Keeps every pixel's samples in tiers by brightness and scales each tier by its support among the neighbours (DESIGN.md 7.10): -o receives the resolved image (with --denoise: the denoiser's source)", 0, [](const char *) { cpu_config.firefly_filter = 1; } });
	o.push_back({ nullptr, "firefly-tiers", "With --firefly-filter: number of tiers (2..8, default 6)", 1, [&cl](const char * v) {
		int n = parse_int(v, "--firefly-tiers");
		if (n < 2 || n > 8) die("--firefly-tiers must be between 2 and 8");
		cpu_config.firefly_tiers = n; cl.firefly_option = true;
	} });
	o.push_back({ nullptr, "firefly-start", "With --firefly-filter: the luminance the lowest tier stands for; tier j stands for 8^j times it (default 1)", 1, [&cl](const char * v) {
		float b = parse_float(v, "--firefly-start");
		if (!(b > 0.0f && b < 1e30f)) die("--firefly-start must be finite and above 0");
		cpu_config.firefly_start = b; cl.firefly_option = true;
	} });
	o.push_back({ nullptr, "firefly-support", "With --firefly-filter: the number of neighbouring samples that keeps a tier whole (above 1, default 4)", 1, [&cl](const char * v) {
		float k = parse_float(v, "--firefly-support");
		if (!(k > 1.0f && k < 1e30f)) die("--firefly-support must be finite and above 1");
		cpu_config.firefly_support = k; cl.firefly_option = true;
	} });
	o.push_back({ nullptr, "firefly-auto-start", "With --firefly-filter: takes the lowest tier's luminance from the frame's own exposure after a few pilot samples, then starts over (DESIGN.md 7.10.1); replaces --firefly-start unless no pixel is lit", 0, [](const char *) { cpu_config.firefly_auto_start = 1; } });
	o.push_back({ nullptr, "firefly-start-shift", "With --firefly-auto-start: the start is 2^(median exponent of the luminance + n), n in -16 .. 16 (default 0)", 1, [&cl](const char * v) {
		int n = parse_int(v, "--firefly-start-shift");
		if (n < -16 || n > 16) die("--firefly-start-shift must be between -16 and 16");
		cpu_config.firefly_start_shift = n; cl.firefly_auto_option = true;
	} });
	o.push_back({ nullptr, "firefly-pilot", "With --firefly-auto-start: the number of pilot samples the exposure is measured on (at least 2, default 4); they are discarded", 1, [&cl](const char * v) {
		int n = parse_int(v, "--firefly-pilot");
		if (n < 2 || n > 1000000) die("--firefly-pilot must be at least 2 (sample 1 overwrites sample 0)");
		cpu_config.firefly_pilot_samples = n; cl.firefly_auto_option = true;
	} });
	o.push_back({ nullptr, "noise-robust", "With --firefly-filter and --noise-target or --noise-map: the noise estimate and --adaptive leave out the pixels the firefly filter holds back (DESIGN.md 7.10.2)", 0, [](const char *) { cpu_config.noise_robust = 1; } });
	o.push_back({ nullptr, "noise-held-fraction", "With --noise-robust: a pixel is held when more than this fraction of its brightness is held back (inside (0, 1), default 0.25)", 1, [&cl](const char * v) {
		float t = parse_float(v, "--noise-held-fraction");
		if (!(t > 0.0f && t < 1.0f)) die("--noise-held-fraction must lie inside (0, 1)");
		cpu_config.noise_held_fraction = t; cl.noise_robust_option = true;
	} });
	o.push_back({ nullptr, "firefly-map", "With --firefly-filter: writes the luminance held back per pixel as a one-channel EXR", 1, [&cl](const char * v) { cl.firefly_map = v; cl.firefly_option = true; } });
	o.push_back({ nullptr, "firefly-unfiltered", "With --firefly-filter: also writes the plain image to <file> (ppm, exr)", 1, [&cl](const char * v) { cl.firefly_unfiltered = v; cl.firefly_option = true; } });
	o.push_back({ nullptr, "sample-map", "Writes the number of samples every pixel's mean stands for as a one-channel EXR", 1, [&cl](const char * v) { cl.sample_map = v; } });
	o.push_back({ nullptr, "force-rebuild", "BVH will not be loaded from disk but rebuilt from scratch", 0, [](const char *) { cpu_config.bvh_force_rebuild = true; } });
	o.push_back({ "O",  "optimize",    "Enables or disables BVH optimization post-processing step", 1, [](const char * v) { cpu_config.enable_bvh_optimization = parse_bool(v); } });
	o.push_back({ "Ot", "opt-time",    "Sets time limit for BVH optimization (milliseconds, as the reference stores it)", 1, [](const char * v) { cpu_config.bvh_optimizer_max_time = parse_int(v, "--opt-time"); } });
	o.push_back({ "Ob", "opt-batches", "Sets a limit on the maximum number of batches used in BVH optimization", 1, [](const char * v) { cpu_config.bvh_optimizer_max_num_batches = parse_int(v, "--opt-batches"); } });
	o.push_back({ nullptr, "sah-node",   "Sets the SAH cost of an internal BVH node", 1, [](const char * v) { cpu_config.sah_cost_node = parse_float(v, "--sah-node"); } });
	o.push_back({ nullptr, "sah-leaf",   "Sets the SAH cost of a leaf BVH node",      1, [](const char * v) { cpu_config.sah_cost_leaf = parse_float(v, "--sah-leaf"); } });
	o.push_back({ nullptr, "sbvh-alpha", "Sets the SBVH alpha constant. An alpha of 1 results in a regular BVH, alpha of 0 results in full SBVH", 1, [](const char * v) { cpu_config.sbvh_alpha = parse_float(v, "--sbvh-alpha"); } });
	o.push_back({ nullptr, "mipmap",     "Enables or disables texture mipmapping",    1, [](const char * v) { gpu_config.enable_mipmapping = parse_bool(v); } });
	o.push_back({ nullptr, "mip-filter", "Sets the downsampling filter for creating mipmaps. Supported options: box, lanczos, kaiser", 1, [](const char * v) {
		if      (strcmp(v, "box")     == 0) cpu_config.mipmap_filter = MipmapFilterType::BOX;
		else if (strcmp(v, "lanczos") == 0) cpu_config.mipmap_filter = MipmapFilterType::LANCZOS;
		else if (strcmp(v, "kaiser")  == 0) cpu_config.mipmap_filter = MipmapFilterType::KAISER;
		else die(std::string("'") + v + "' is not a recognized Mipmap Filter!");
	} });
	o.push_back({ "c", "compress",  "Enables or disables texture block compression (BC1, decoded in the shade kernels; default true, as in the reference)", 1, [](const char * v) { cpu_config.enable_block_compression = parse_bool(v); } });
	o.push_back({ nullptr, "device",    "HIP device ordinal to render on", 1, [&cl](const char * v) { cl.device = parse_int(v, "--device"); } });
	o.push_back({ nullptr, "devices",   "Comma-separated HIP device ordinals: the frame is split into row tiles over them (an ordinal may repeat: contexts sharing a GPU)", 1, [&cl](const char * v) {
		cl.devices.clear();
		std::string list(v);
		for (size_t at = 0; at <= list.size(); ) {
			size_t comma = list.find(',', at); if (comma == std::string::npos) comma = list.size();
			cl.devices.push_back(parse_int(list.substr(at, comma - at).c_str(), "--devices"));
			at = comma + 1;
		}
	} });
	o.push_back({ nullptr, "bvh-cache", "Enables or disables reading and writing <mesh>.bvh cache files", 1, [](const char * v) { cpu_config.enable_bvh_cache = parse_bool(v); } });
	o.push_back({ nullptr, "merge-static", "Static instances flattened into one tree: 1 (default), 2 (no spatial splits), 3 (identity instances only), 0 (one BLAS per mesh under the TLAS, as the reference)", 1, [](const char * v) {
		cpu_config.merge_static = parse_int(v, "--merge-static");
		if (cpu_config.merge_static < 0 || cpu_config.merge_static > 3) die("--merge-static must be 0, 1, 2 or 3");
	} });
	o.push_back({ nullptr, "alpha-masks", "Alpha-tested cut-outs: materials whose albedo file has a varying alpha channel get an opacity mask from it", 0, [](const char *) { cpu_config.alpha_masks = 1; } });
	o.push_back({ nullptr, "batch",     "Samples per submission to the device (1..16)", 1, [&cl](const char * v) {
		cl.batch = parse_int(v, "--batch");
		if (cl.batch < 1 || cl.batch > 16) die("--batch must be between 1 and 16");
	} });
	o.push_back({ nullptr, "print-config", "Prints the configuration the command line amounts to and exits", 0, [&cl](const char *) { cl.print_config = true; } });
	o.push_back({ "h", "help", "Displays this message", 0, [&cl](const char *) { cl.help = true; } });
	return o;
}

void print_help(const std::vector<Option> & options) {
	for (const Option & o : options) {
		if (o.short_name) printf("-%s,\t--%-16s%s\n", o.short_name, o.long_name, o.help);
		else              printf("\t--%-16s%s\n", o.long_name, o.help);
	}
}

void parse_command_line(int argc, char ** argv, CommandLine & cl) {
	std::vector<Option> options = make_options(cl);
	for (int i = 1; i < argc; i++) {
		const char * arg = argv[i];
		if (arg[0] != '-') { // without an explicit option: a scene file
			cpu_config.scene_filenames.push_back(arg);
			continue;
		}
		bool long_form = arg[1] == '-';
		const char * name = arg + (long_form ? 2 : 1);
		const Option * match = nullptr;
		for (const Option & o : options) {
			const char * candidate = long_form ? o.long_name : o.short_name;
			if (candidate && strcmp(candidate, name) == 0) { match = &o; break; }
		}
		if (!match) {
			printf("Unrecognized command line option '%s'\nUse --help for a list of valid options\n", arg);
			continue;
		}
		if (i + match->argument_count >= argc) {
			printf("Not enough arguments provided to option '%s'!\n", match->long_name);
			break; // the reference stops parsing here
		}
		match->apply(match->argument_count ? argv[i + 1] : nullptr);
		i += match->argument_count;
	}
	if (cl.help) {
		print_help(options);
		exit(0);
	}
	if (cpu_config.adaptive_sampling && !(cpu_config.noise_target > 0.0f)) die("--adaptive needs --noise-target: the cells are selected by it");
	if (cl.denoise_option && !cpu_config.denoise) die("--denoise-iterations / --denoise-noisy need --denoise");
	if (!cl.denoise_noisy.empty() && cl.denoise_noisy == cpu_config.output_filename) die("--denoise-noisy names the output file: the denoised image goes there");
	if (cl.firefly_option && !cpu_config.firefly_filter) die("--firefly-tiers / --firefly-start / --firefly-support / --firefly-map / --firefly-unfiltered need --firefly-filter");
	if (cpu_config.firefly_auto_start && !cpu_config.firefly_filter) die("--firefly-auto-start needs --firefly-filter");
	if (cl.firefly_auto_option && !cpu_config.firefly_auto_start) die("--firefly-start-shift / --firefly-pilot need --firefly-auto-start");
	if (cpu_config.noise_robust && !cpu_config.firefly_filter) die("--noise-robust needs --firefly-filter: it follows the filter's judgement");
	if (cpu_config.noise_robust && !(cpu_config.noise_target > 0.0f) && cl.noise_map.empty()) die("--noise-robust needs --noise-target or --noise-map: it is an estimate nobody asks for");
	if (cl.noise_robust_option && !cpu_config.noise_robust) die("--noise-held-fraction needs --noise-robust");
	if (!cl.firefly_unfiltered.empty() && cl.firefly_unfiltered == cpu_config.output_filename) die("--firefly-unfiltered names the output file: the resolved image goes there");
	if (!cl.firefly_map.empty() && (cl.firefly_map == cpu_config.output_filename || cl.firefly_map == cl.firefly_unfiltered)) die("--firefly-map names a file another image goes to");
	if (cl.print_config) { // one line, floats as bit patterns; the form oracle/ref/ref_scene_harness.cpp writes for the reference's Args::parse
		auto bits = [](float f) { unsigned u; memcpy(&u, &f, 4); return u; };
		std::string scenes;
		for (const std::string & s : cpu_config.scene_filenames) { if (!scenes.empty()) scenes += '|'; scenes += s; }
		printf("integrator=%d width=%d height=%d num_bounces=%d samples=%d output=\"%s\" scenes=\"%s\" sky=\"%s\" bvh_type=%d nee=%d mis=%d force_rebuild=%d "
		       "optimize=%d opt_time=%d opt_batches=%d sah_node=%08x sah_leaf=%08x sbvh_alpha=%08x mipmap=%d mip_filter=%d compress=%d\n",
		       int(cpu_config.integrator), cpu_config.initial_width, cpu_config.initial_height, gpu_config.num_bounces, cpu_config.output_sample_index,
		       cpu_config.output_filename.c_str(), scenes.c_str(), cpu_config.sky_filename.c_str(), int(cpu_config.bvh_type),
		       int(gpu_config.enable_next_event_estimation), int(gpu_config.enable_multiple_importance_sampling), int(cpu_config.bvh_force_rebuild),
		       int(cpu_config.enable_bvh_optimization), cpu_config.bvh_optimizer_max_time, cpu_config.bvh_optimizer_max_num_batches,
		       bits(cpu_config.sah_cost_node), bits(cpu_config.sah_cost_leaf), bits(cpu_config.sbvh_alpha), int(gpu_config.enable_mipmapping),
		       int(cpu_config.mipmap_filter), int(cpu_config.enable_block_compression));
		exit(0);
	}
}

// --noise-target / --noise-map: asked at burst boundaries (every `interval` samples), since the answer drains the wavefront
struct NoiseStop {
	bool active = false, warned = false, reached = false;
	int interval = 1, next_check = 0;
	NoiseEstimate last; bool have = false;
	bool adaptive = false;               // --adaptive: every check that goes on selects the cells the next passes render
	std::vector<double> active_share;    // ... and notes the share of the cells that stayed active
	template<typename Renderer> bool should_stop(Renderer & r, int sample_index) {   // after a render call
		if (!active || sample_index < cpu_config.noise_min_samples || sample_index < next_check) return false;
		next_check = sample_index + interval;
		last = r.noise(); have = true;
		reached = last.pixels > 0 && last.figure <= double(cpu_config.noise_target);
		if constexpr (std::is_same<Renderer, Pathtracer>::value) if (adaptive && !reached) {
			AdaptiveSelection chosen = r.select_adaptive(cpu_config.noise_target);
			active_share.push_back(double(chosen.active_cells) / double(chosen.cells));
		}
		return reached;
	}
	// --adaptive's lines of the final report, --sample-map
	void report_samples(Pathtracer & r, const std::string & map_file, int pitch, int width, int height) {
		if (!adaptive && map_file.empty()) return;
		std::vector<float> counts;
		double mean = r.sample_counts(&counts);
		if (adaptive) {
			// (w counts the samples past sample 0, which sample 1 overwrites: a pixel with w samples in its mean was rendered w + 1 times)
			printf("Adaptive: %.3f samples per pixel on average; %.1f %% of the cells active at the end; per check:", mean + 1.0, active_share.empty() ? 100.0 : 100.0 * active_share.back());
			for (double share : active_share) printf(" %.3f", share);
			printf("\n");
		}
		if (!map_file.empty()) {
			if (!EXRExporter::save_luminance(map_file, pitch, width, height, counts)) die("failed to write '" + map_file + "'");
			printf("Wrote %s\n", map_file.c_str());
		}
	}
	template<typename Renderer> void report(Renderer & r, int sample_index, const std::string & map_file, int pitch, int width, int height) {
		if (active) {
			if (!reached) { last = r.noise(); have = true; reached = last.pixels > 0 && last.figure <= double(cpu_config.noise_target); }
			if (last.robust) printf("Noise (firefly-robust, %lld pixels held): figure %.6g (mean %.6g, target %.6g) after sample %d; %s\n", last.held_pixels, last.figure, last.mean,
			                        double(cpu_config.noise_target), sample_index, reached ? "target reached" : "stopped at the sample cap");
			else printf("Noise: figure %.6g (mean %.6g, target %.6g) after sample %d; %s\n", last.figure, last.mean, double(cpu_config.noise_target), sample_index,
			            reached ? "target reached" : "stopped at the sample cap");
		}
		if (!map_file.empty()) {
			std::vector<float> map;
			const NoiseEstimate mapped = r.noise(&map);
			if (mapped.robust && !active) printf("Noise map: firefly-robust, %lld pixels held\n", mapped.held_pixels);
			for (float & v : map) if (v < 0.0f) v = 0.0f;   // (no part, non-finite, held)
			if (!EXRExporter::save_luminance(map_file, pitch, width, height, map)) die("failed to write '" + map_file + "'");
			printf("Wrote %s\n", map_file.c_str());
		}
	}
};

double seconds_since(std::chrono::steady_clock::time_point t0) {
	return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

} // namespace

int main(int argc, char ** argv) {
	CommandLine cl;
	parse_command_line(argc, argv, cl);

	if (cpu_config.scene_filenames.empty()) die("no scene file given (use -s <scene.xml|.obj|.ply>); --help lists the options");
	if (cpu_config.output_sample_index == CPUConfig::INVALID_SAMPLE) cpu_config.output_sample_index = 1; // no window to keep open: one sample

	try {
		auto t0 = std::chrono::steady_clock::now();
		Scene scene;
		NoiseStop noise;
		const bool noise_asked = cpu_config.noise_target > 0.0f || !cl.noise_map.empty();
		if (noise_asked && (gpu_config.enable_svgf || cpu_config.integrator == IntegratorType::AO)) {   // neither keeps second moments
			fprintf(stderr, "WARNING: --noise-target / --noise-map need plain path tracing (no SVGF, no AO integrator): ignored, rendering to -N\n");
			cpu_config.noise_target = 0.0f; cl.noise_map.clear();
		}
		if ((cpu_config.adaptive_sampling || !cl.sample_map.empty()) && (gpu_config.enable_svgf || cpu_config.integrator == IntegratorType::AO)) {
			fprintf(stderr, "WARNING: --adaptive / --sample-map need plain path tracing (no SVGF, no AO integrator): ignored\n");
			cpu_config.adaptive_sampling = 0; cl.sample_map.clear();
		}
		if (cpu_config.adaptive_sampling && cl.devices.size() > 1) {   // (once: the tile split has no pixel lists)
			fprintf(stderr, "WARNING: --adaptive does not work across --devices: rendering uniformly\n");
			cpu_config.adaptive_sampling = 0;
		}
		if (cpu_config.denoise && (gpu_config.enable_svgf || cpu_config.integrator == IntegratorType::AO)) {   // neither keeps second moments
			fprintf(stderr, "WARNING: --denoise needs plain path tracing (no SVGF, no AO integrator): ignored, writing the plain image\n");
			cpu_config.denoise = 0;
		}
		if (cpu_config.denoise && cl.devices.size() > 1) {   // (moments and guides are not gathered)
			fprintf(stderr, "WARNING: --denoise does not work across --devices: writing the plain image\n");
			cpu_config.denoise = 0;
		}
		if (cpu_config.firefly_filter && (gpu_config.enable_svgf || cpu_config.integrator == IntegratorType::AO)) {   // neither splats: their accumulate keeps no moments
			fprintf(stderr, "WARNING: --firefly-filter needs plain path tracing (no SVGF, no AO integrator): ignored, writing the plain image\n");
			cpu_config.firefly_filter = 0;
		}
		if (cpu_config.firefly_filter && cl.devices.size() > 1) {   // (the tiers are not gathered)
			fprintf(stderr, "WARNING: --firefly-filter does not work across --devices: writing the plain image\n");
			cpu_config.firefly_filter = 0;
		}
		if (cpu_config.noise_robust && !cpu_config.firefly_filter) {   // (switched off above: the robust estimate follows the filter's resolve)
			fprintf(stderr, "WARNING: --noise-robust needs the firefly filter: keeping the plain noise estimate\n");
			cpu_config.noise_robust = 0;
		}
		if (!cl.sample_map.empty() && cl.devices.size() > 1) { fprintf(stderr, "WARNING: --sample-map does not work across --devices: ignored\n"); cl.sample_map.clear(); }
		noise.active = cpu_config.noise_target > 0.0f;
		noise.adaptive = noise.active && cpu_config.adaptive_sampling != 0;
		if ((!cl.noise_map.empty() || !cl.sample_map.empty()) && !noise.active) cpu_config.noise_target = 1e-30f;   // (keeps the moments; a target nothing reaches, and no stop is asked for)
		if (cl.devices.size() > 1) { // one frame over several GPUs
			if (cpu_config.integrator == IntegratorType::AO) die("--devices: the tile split exists for the path tracer");
			FrameSplit split(cpu_config.initial_width, cpu_config.initial_height, scene, cl.devices);
			printf("Initialization: %.0f ms (%d ranks)\n", seconds_since(t0) * 1e3, split.world());
			auto t1 = std::chrono::steady_clock::now();
			int target = cpu_config.output_sample_index;
			noise.interval = 8 * cl.batch;
			while (true) {
				split.update(0.0f);
				int remaining = target - split.sample_index() + 1;
				if (cl.batch > 1 && split.sample_index() > 0 && remaining > 1) split.render_samples(remaining < cl.batch ? remaining : cl.batch);
				else split.render();
				if (split.sample_index() >= target || noise.should_stop(split, split.sample_index())) break;
			}
			split.read_framebuffer(); // waits for the devices
			printf("Rendered sample %d at %dx%d in %.1f ms\n", split.sample_index(), split.front().screen_width, split.front().screen_height, seconds_since(t1) * 1e3);
			noise.report(split, split.sample_index(), cl.noise_map, split.front().screen_pitch, split.front().screen_width, split.front().screen_height);
			split.save_image(cpu_config.output_filename);
			printf("Wrote %s\n", cpu_config.output_filename.c_str());
			return 0;
		}
		if (cl.devices.size() == 1) cl.device = cl.devices[0];
		std::unique_ptr<Integrator> integrator;
		if (cpu_config.integrator == IntegratorType::AO) integrator = std::make_unique<AO>        (cpu_config.initial_width, cpu_config.initial_height, scene, cl.device);
		else                                             integrator = std::make_unique<Pathtracer>(cpu_config.initial_width, cpu_config.initial_height, scene, cl.device);
		printf("Initialization: %.0f ms\n", seconds_since(t0) * 1e3);

		Pathtracer * pathtracer = dynamic_cast<Pathtracer *>(integrator.get());
		auto t1 = std::chrono::steady_clock::now();
		int target = cpu_config.output_sample_index;
		// A headless render of `-N n` samples is a batch job: nothing is read before the last sample. Declared to the device library
		// (rt_set_stream_batch), up to eight of its submissions enter the merged wavefront together and walk their bounces side by side
		// instead of one after the other (the same image). Not for SVGF frames (each inherits its predecessor's g-buffers).
		if (pathtracer && integrator->ctx && cl.batch > 1 && target + 1 > cl.batch && !gpu_config.enable_svgf) {
			const long long submissions = (long long)(target + cl.batch) / cl.batch;
			const long long burst = submissions < 8 ? submissions : 8;
			noise.interval = int(burst) * cl.batch;
			if (rt_set_frame_pipelining(integrator->ctx, 1) != RT_OK || rt_set_stream_batch(integrator->ctx, burst * cl.batch * (long long)cpu_config.initial_width * cpu_config.initial_height) != RT_OK)
				die(std::string("ERROR: ") + rt_last_error(integrator->ctx));
		}
		while (true) {
			integrator->update(0.0f);
			int remaining = target - integrator->sample_index + 1;
			if (pathtracer && cl.batch > 1 && integrator->sample_index > 0 && remaining > 1) {
				pathtracer->render_samples(remaining < cl.batch ? remaining : cl.batch);
			} else {
				integrator->render();
			}
			if (integrator->sample_index >= target || (pathtracer && noise.should_stop(*pathtracer, integrator->sample_index))) break;
		}
		integrator->read_framebuffer(); // waits for the device
		double render_s = seconds_since(t1);
		printf("Rendered sample %d at %dx%d in %.1f ms\n", integrator->sample_index, integrator->screen_width, integrator->screen_height, render_s * 1e3);
		if (pathtracer) noise.report(*pathtracer, integrator->sample_index, cl.noise_map, integrator->screen_pitch, integrator->screen_width, integrator->screen_height);
		if (pathtracer) noise.report_samples(*pathtracer, cl.sample_map, integrator->screen_pitch, integrator->screen_width, integrator->screen_height);

		const bool resolve = pathtracer && cpu_config.firefly_filter;
		if (resolve) {
			auto save_rgb = [&](const std::string & file, const std::vector<float> & rgba) {
				std::vector<Vector3> rgb(rgba.size() / 4);
				for (size_t i = 0; i < rgb.size(); i++) rgb[i] = Vector3(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]);
				std::string error;
				if (!Exporters::save(file, integrator->screen_pitch, integrator->screen_width, integrator->screen_height, rgb, &error)) die(error);
			};
			if (!cl.firefly_unfiltered.empty()) { save_rgb(cl.firefly_unfiltered, integrator->read_framebuffer()); printf("Wrote %s\n", cl.firefly_unfiltered.c_str()); }
			auto t2 = std::chrono::steady_clock::now();
			const std::vector<float> resolved = pathtracer->resolve_fireflies();
			double held = 0.0, kept = 0.0;   // over the valid pixels, in luminance
			std::vector<float> plane(resolved.size() / 4, 0.0f);
			for (int y = 0; y < integrator->screen_height; y++) for (int x = 0; x < integrator->screen_width; x++) {
				const size_t i = size_t(y) * integrator->screen_pitch + x;
				plane[i] = resolved[4 * i + 3];
				if (resolved[4 * i + 3] >= 0.0f) { held += resolved[4 * i + 3]; kept += 0.299 * resolved[4 * i] + 0.587 * resolved[4 * i + 1] + 0.114 * resolved[4 * i + 2]; }
			}
			if (cpu_config.firefly_auto_start && pathtracer->firefly_start_measured && pathtracer->firefly_start_in_force > 0.0f)
				printf("Firefly start: %g from the exposure of %d pilot samples (median exponent %d with shift %d; %lld samples discarded)\n", double(pathtracer->firefly_start()),
				       cpu_config.firefly_pilot_samples, pathtracer->firefly_median_exponent, cpu_config.firefly_start_shift, pathtracer->firefly_pilot_samples_discarded);
			else if (cpu_config.firefly_auto_start) printf("Firefly start: %g (no exposure could be measured)\n", double(pathtracer->firefly_start()));
			printf("Firefly filter: %d tiers from %g, support %g; %.3f %% of the luminance held back; resolve %.1f ms\n", cpu_config.firefly_tiers, double(pathtracer->firefly_start()), cpu_config.firefly_support,
			       held + kept > 0.0 ? 100.0 * held / (held + kept) : 0.0, seconds_since(t2) * 1e3);
			if (!cl.firefly_map.empty()) {
				if (!EXRExporter::save_luminance(cl.firefly_map, integrator->screen_pitch, integrator->screen_width, integrator->screen_height, plane)) die("failed to write '" + cl.firefly_map + "'");
				printf("Wrote %s\n", cl.firefly_map.c_str());
			}
			if (cpu_config.denoise) { if (rt_set_denoise_source(integrator->ctx, RT_DENOISE_SOURCE_RESOLVED) != RT_OK) die(std::string("ERROR: ") + rt_last_error(integrator->ctx)); }
			else save_rgb(cpu_config.output_filename, resolved);
		}
		if (pathtracer && cpu_config.denoise) {
			if (!cl.denoise_noisy.empty()) {
				std::vector<float> rgba = integrator->read_framebuffer();
				std::vector<Vector3> rgb(rgba.size() / 4);
				for (size_t i = 0; i < rgb.size(); i++) rgb[i] = Vector3(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]);
				std::string error;
				if (!Exporters::save(cl.denoise_noisy, integrator->screen_pitch, integrator->screen_width, integrator->screen_height, rgb, &error)) die(error);
				printf("Wrote %s\n", cl.denoise_noisy.c_str());
			}
			auto t2 = std::chrono::steady_clock::now();
			pathtracer->save_denoised_image(cpu_config.output_filename);
			printf("Denoised: %d iterations, filter and export %.1f ms\n", cpu_config.denoise_iterations, seconds_since(t2) * 1e3);
		} else if (!resolve) integrator->save_image(cpu_config.output_filename);
		printf("Wrote %s\n", cpu_config.output_filename.c_str());
	} catch (const std::exception & e) {
		die(std::string("ERROR: ") + e.what());
	}
	return 0;
}
