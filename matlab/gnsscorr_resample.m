function [res, newSettings] = gnsscorr_resample(h, hDst, settings, prototype, centerFreq, interp, decim, targetRms, nOutputs)
%GNSSCORR_RESAMPLE  A record at a rational multiple of its rate, on the GPU.
%   [res, newSettings] = gnsscorr_resample(h, hDst, settings, prototype, centerFreq, interp, decim, targetRms, nOutputs)
%   writes the record of context h at interp / decim times its rate into the record of context hDst (another context on the same
%   device; any size and format), the band around centerFreq (Hz) taken to DC, by one 'resample' command.
%     prototype  the REAL low-pass of the caller at the rate fs * interp with gain interp at DC, e.g.
%                interp * fir1(16 * max(interp, decim), 0.8 * min(1, interp / decim) / interp); the wrapper moves it to the band:
%                g(k) = prototype(k) * exp(+j 2 pi fUsed (k - 1) / (fs * interp)), fUsed the frequency the NCO's 64-bit step per tick
%                gives centerFreq.  Output m (0-based) lines up with tick m * decim, input sample m * decim / interp:
%                firstTick0 = floor((T - 1) / 2).
%     targetRms  [] (default): gain 1.  Else the rms a stored component should have: the command runs on the first
%                min(nOutputs, 65536) outputs, the taps are scaled by targetRms / the rms sumSq gives, and the range runs with them.
%     nOutputs   [] (default): every output with a record sample under it, up to hDst's capacity.
%   res: clipped, sumSq, carrFreq, nOutputs, outRate.  newSettings: settings with samplingFreq = outRate and IF = centerFreq - fUsed,
%   and the fields rsGain, rsDelay (the filter's residual delay in ticks: 0 for an odd T), rsInterp and rsDecim; a code phase found
%   on hDst's record maps back as sample * decim / interp.  The same steps as receiver.resample_record of the Python package.
%   Written for this repository; not a copy of any reference file.
if nargin < 8, targetRms = []; end
if nargin < 9, nOutputs = []; end
fs = settings.samplingFreq;
rate = fs * interp;
T = numel(prototype);
step = round(centerFreq / rate * (2^64));                                         % whole already wherever |centerFreq / rate| >= 2^-11
fUsed = step * (2^(-64)) * rate;
ang = 2 * pi * fUsed * (0:T-1) / rate;
lp = reshape(prototype, 1, T);
taps = [lp .* cos(ang); lp .* sin(ang)];                                       % 2 x T: re; im
first = floor((T - 1) / 2);
gain = 1;
if ~isempty(targetRms)
    if isempty(nOutputs)
        r = gnsscorr_mex('resample', h, hDst, taps, interp, decim, centerFreq, 0, first);
        nTrial = min(r(4), 65536);
    else
        nTrial = min(nOutputs, 65536);
    end
    r = gnsscorr_mex('resample', h, hDst, taps, interp, decim, centerFreq, 0, first, nTrial);
    components = 1 + (settings.fileType == 2);
    rmsNow = sqrt(r(2) / (components * r(4)));
    if ~(rmsNow > 0)
        error('gnsscorr:usage', 'gnsscorr_resample: the band holds nothing to scale');
    end
    gain = targetRms / rmsNow;
end
r = gnsscorr_mex('resample', h, hDst, gain * taps, interp, decim, centerFreq, 0, first, nOutputs);
res = struct('clipped', r(1), 'sumSq', r(2), 'carrFreq', r(3), 'nOutputs', r(4), 'outRate', r(5));
newSettings = settings;
newSettings.samplingFreq = r(5);
newSettings.IF = centerFreq - fUsed;
newSettings.rsGain = gain;
newSettings.rsDelay = (T - 1) / 2 - first;
newSettings.rsInterp = interp;
newSettings.rsDecim = decim;
end
