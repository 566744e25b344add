// The part of the C shim (capi.cpp) that the command-line front end uses too: the config keys whose values are lists of numbers, and the shim's error text.
#pragma once

extern "C" {
// fog ("off", or the box "minx,miny,minz,maxx,maxy,maxz"), fog_sigma_a and fog_sigma_s (one number or three), fog_density ("off" or a gridvolume
// file's path); -1 with a message for anything else
int grt_config_set_string(const char * key, const char * value);
const char * grt_last_error();
}
